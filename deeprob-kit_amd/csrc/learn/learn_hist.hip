// libdeeprob_learn.so, histograms of float columns: the bin codes of numpy's uniform bins, the counts of the codes and the
// G statistic of a pair of coded columns, segmented over the tasks of one generation (include/deeprob_learn.h, section
// "histograms of float columns").  Built with -ffp-contract=off like learn.hip: an edge is one float32 multiply and one
// float32 add, and every float64 expression is evaluated operation by operation in the order the header states.
#include "learn_common.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdeeprob_learn is written for gfx950 (MI355X)"
#endif

namespace {

using dpl_detail::common_ok;
using dpl_detail::kMaxGrid;
using dpl_detail::kThreads;
using dpl_detail::set_error;
using dpl_detail::sum_in_order;
constexpr double kEps32 = 1.1920928955078125e-07;   // np.finfo(np.float32).eps (gvs.py:193)

// ---- bin codes -------------------------------------------------------------------------------------------------------
// edge i < bins of np.linspace(lo, hi, bins + 1) in float32; the last edge (hi itself) is never asked for: a value
// never moves past bin bins - 1
__device__ __forceinline__ float edge_of(int i, float step, float lo) {
    const float scaled = (float)i * step;
    return scaled + lo;
}

__global__ __launch_bounds__(kThreads) void hist_codes_kernel(
    const float *__restrict__ xf, int64_t n_rows, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ item_col, const int64_t *__restrict__ item_row_off, const int32_t *__restrict__ item_n,
    const int64_t *__restrict__ item_out_off, const float *__restrict__ item_lo, const float *__restrict__ item_hi,
    const int32_t *__restrict__ item_bins, const int32_t *__restrict__ block_item, const int32_t *__restrict__ block_row0,
    uint16_t *__restrict__ codes) {
    const int item = block_item[blockIdx.x];
    const int i = block_row0[blockIdx.x] + threadIdx.x;
    if (i >= item_n[item]) return;
    const float v = xf[(int64_t)item_col[item] * n_rows + row_index[item_row_off[item] + i]];
    const float lo = item_lo[item], hi = item_hi[item];
    const int bins = max(item_bins[item], 1);
    const float span = hi - lo;
    const float step = span / (float)bins;
    // the guess (multiply and truncate, in float64), then the edges decide: the largest bin whose left edge is <= v
    const double guess = ((double)v - (double)lo) / (double)span * (double)bins;
    int b = guess >= (double)(bins - 1) ? bins - 1 : (guess > 0.0 ? (int)guess : 0);
    while (b > 0 && v < edge_of(b, step, lo)) --b;
    while (b < bins - 1 && v >= edge_of(b + 1, step, lo)) ++b;
    codes[item_out_off[item] + i] = (uint16_t)b;
}

// ---- counts of the codes ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void code_counts_kernel(
    const uint16_t *__restrict__ codes, const int64_t *__restrict__ item_code_off, const int32_t *__restrict__ item_n,
    const int32_t *__restrict__ item_bins, const int64_t *__restrict__ item_count_off, int32_t *__restrict__ counts) {
    __shared__ int cnt[DPL_HIST_MAX_BINS];
    const int64_t item = blockIdx.x;
    const int bins = min(item_bins[item], DPL_HIST_MAX_BINS), n = item_n[item];
    for (int b = threadIdx.x; b < bins; b += kThreads) cnt[b] = 0;
    __syncthreads();
    const uint16_t *code = codes + item_code_off[item];
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const int b = code[r];
        if (b < bins) atomicAdd(&cnt[b], 1);
    }
    __syncthreads();
    int32_t *out = counts + item_count_off[item];
    for (int b = threadIdx.x; b < bins; b += kThreads) out[b] = cnt[b];
}

// ---- G statistic of two coded columns --------------------------------------------------------------------------------
// Dynamic LDS: the marginals (float64, ba + bb of them) first, then the joint table (int32, ba * bb cells); the entry
// sizes it for the largest table of the launch.
__global__ __launch_bounds__(kThreads) void pair_g_codes_kernel(
    const uint16_t *__restrict__ codes, const int64_t *__restrict__ pair_off_a, const int64_t *__restrict__ pair_off_b,
    const int32_t *__restrict__ pair_n, const int32_t *__restrict__ pair_bins_a, const int32_t *__restrict__ pair_bins_b,
    int max_bins_sum, int max_cells, double *__restrict__ g) {
    extern __shared__ double lds[];
    __shared__ double part[kThreads];
    const int64_t q = blockIdx.x;
    const int ba = pair_bins_a[q], bb = pair_bins_b[q], n = pair_n[q], cells = ba * bb;
    if (ba < 1 || bb < 1 || ba + bb > max_bins_sum || cells > max_cells) {      // (block-uniform: a table the launch's LDS
        if (threadIdx.x == 0) g[q] = NAN;                                       // was not sized for is not touched)
        return;
    }
    double *m1 = lds, *m2 = lds + ba;
    int *joint = reinterpret_cast<int *>(lds + ba + bb);
    for (int c = threadIdx.x; c < cells; c += kThreads) joint[c] = 0;
    __syncthreads();
    const uint16_t *ca = codes + pair_off_a[q], *cb = codes + pair_off_b[q];
    for (int r = threadIdx.x; r < n; r += kThreads) {
        const int a = ca[r], b = cb[r];
        if (a < ba && b < bb) atomicAdd(&joint[a * bb + b], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ba + bb; i += kThreads) {
        double s;
        if (i < ba) {
            s = (double)joint[i * bb] + kEps32;
            for (int b = 1; b < bb; ++b) s += (double)joint[i * bb + b] + kEps32;
        } else {
            const int b = i - ba;
            s = (double)joint[b] + kEps32;
            for (int a = 1; a < ba; ++a) s += (double)joint[a * bb + b] + kEps32;
        }
        lds[i] = s;
    }
    __syncthreads();
    double mine = 0.0;
    for (int c = threadIdx.x; c < cells; c += kThreads) {
        const int a = c / bb, b = c - a * bb;
        const double h = (double)joint[c] + kEps32;
        const double e = m1[a] * m2[b] / (double)n;
        mine += h * log(h / e);
    }
    const double total = sum_in_order(part, mine);
    if (threadIdx.x == 0) g[q] = 2.0 * total;
}

}  // namespace

extern "C" {

int dpl_hist_codes(const float *xf, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                   const int32_t *item_col, const int64_t *item_row_off, const int32_t *item_n,
                   const int64_t *item_out_off, const float *item_lo, const float *item_hi, const int32_t *item_bins,
                   int64_t n_items, const int32_t *block_item, const int32_t *block_row0, int64_t n_blocks,
                   uint16_t *codes, int64_t n_out, void *stream) {
    if (!common_ok(xf, n_rows, n_cols, row_index, n_index, "dpl_hist_codes")) return DPL_EINVAL;
    DPL_REQUIRE(item_col && item_row_off && item_n && item_out_off && item_lo && item_hi && item_bins && block_item &&
                    block_row0 && codes, "dpl_hist_codes: null argument");
    DPL_REQUIRE(n_items >= 1 && n_blocks >= 1 && n_blocks <= kMaxGrid && n_out >= 1,
                "dpl_hist_codes: n_items = %lld, n_blocks = %lld, n_out = %lld out of domain", (long long)n_items,
                (long long)n_blocks, (long long)n_out);
    DPL_LAUNCH("dpl_hist_codes", hist_codes_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, xf, n_rows,
               row_index, item_col, item_row_off, item_n, item_out_off, item_lo, item_hi, item_bins, block_item, block_row0,
               codes);
    return DPL_OK;
}

int dpl_code_counts(const uint16_t *codes, int64_t n_codes, const int64_t *item_code_off, const int32_t *item_n,
                    const int32_t *item_bins, const int64_t *item_count_off, int64_t n_items, int32_t *counts,
                    int64_t n_counts, void *stream) {
    DPL_REQUIRE(codes && item_code_off && item_n && item_bins && item_count_off && counts, "dpl_code_counts: null argument");
    DPL_REQUIRE(n_codes >= 1 && n_items >= 1 && n_items <= kMaxGrid && n_counts >= 1,
                "dpl_code_counts: n_codes = %lld, n_items = %lld, n_counts = %lld out of domain", (long long)n_codes,
                (long long)n_items, (long long)n_counts);
    DPL_LAUNCH("dpl_code_counts", code_counts_kernel, dim3((unsigned)n_items), dim3(kThreads), 0, (hipStream_t)stream, codes,
               item_code_off, item_n, item_bins, item_count_off, counts);
    return DPL_OK;
}

int dpl_pair_g_codes(const uint16_t *codes, int64_t n_codes, const int64_t *pair_off_a, const int64_t *pair_off_b,
                     const int32_t *pair_n, const int32_t *pair_bins_a, const int32_t *pair_bins_b, int64_t n_pairs,
                     int max_bins_sum, int max_cells, double *g, void *stream) {
    DPL_REQUIRE(codes && pair_off_a && pair_off_b && pair_n && pair_bins_a && pair_bins_b && g, "dpl_pair_g_codes: null argument");
    DPL_REQUIRE(n_codes >= 1 && n_pairs >= 1 && n_pairs <= kMaxGrid, "dpl_pair_g_codes: n_codes = %lld, n_pairs = %lld out of domain",
                (long long)n_codes, (long long)n_pairs);
    DPL_REQUIRE(max_cells >= 1 && max_cells <= DPL_HIST_MAX_CELLS && max_bins_sum >= 2 && max_bins_sum <= 2 * DPL_HIST_MAX_BINS,
                "dpl_pair_g_codes: max_cells = %d (<= %d), max_bins_sum = %d (<= %d) out of domain", max_cells, DPL_HIST_MAX_CELLS,
                max_bins_sum, 2 * DPL_HIST_MAX_BINS);
    const size_t lds = (size_t)max_bins_sum * sizeof(double) + (size_t)max_cells * sizeof(int32_t);
    DPL_REQUIRE(lds + kThreads * sizeof(double) <= 65536, "dpl_pair_g_codes: %d marginals and %d cells need %zu bytes of LDS, over "
                "64 KiB with the partial sums", max_bins_sum, max_cells, lds);
    DPL_LAUNCH("dpl_pair_g_codes", pair_g_codes_kernel, dim3((unsigned)n_pairs), dim3(kThreads), lds, (hipStream_t)stream, codes,
               pair_off_a, pair_off_b, pair_n, pair_bins_a, pair_bins_b, max_bins_sum, max_cells, g);
    return DPL_OK;
}

}  // extern "C"
