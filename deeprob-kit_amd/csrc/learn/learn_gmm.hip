// libdeeprob_learn.so, Gaussian-mixture row splits: the density pass and the weighted moments of one EM iteration over
// every listed (task, initialisation) pair of a generation (include/deeprob_learn.h, last section).  Built with
// -ffp-contract=off like the other sources: every float64 expression is evaluated operation by operation in the order the
// header states.
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

// The two data layouts as a policy of the kernels below: the float64 value of one feature of one row.
struct OneHotFeatures {
    using value = uint8_t;
    __device__ __forceinline__ double feature(const uint8_t *__restrict__ x, int64_t n_rows, int row, int col, int val) const {
        const int v = x[(int64_t)col * n_rows + row];
        return val < 0 ? (double)v : (v == val ? 1.0 : 0.0);
    }
};
struct FloatFeatures {
    using value = float;
    __device__ __forceinline__ double feature(const float *__restrict__ xf, int64_t n_rows, int row, int col, int) const {
        return (double)xf[(int64_t)col * n_rows + row];
    }
};

// ---- E-step: a thread per row, W_c through LDS one 32 x 32 tile at a time --------------------------------------------------
template <class Features>
__global__ __launch_bounds__(kThreads) void gmm_estep_kernel(
    const typename Features::value *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index, Features features,
    const int64_t *__restrict__ task_row_off, const int32_t *__restrict__ task_n, const int64_t *__restrict__ task_lab_off,
    const int32_t *__restrict__ task_feat_off, const int32_t *__restrict__ task_f, const int32_t *__restrict__ feat_col,
    const int32_t *__restrict__ feat_val, const int32_t *__restrict__ pair_task, const int32_t *__restrict__ pair_init,
    const int64_t *__restrict__ pair_par_off, const int32_t *__restrict__ block_pair, const int32_t *__restrict__ block_row0,
    int n_comp, const double *__restrict__ par, double *__restrict__ resp, uint8_t *__restrict__ labels,
    double *__restrict__ lse, int64_t n_lab) {
    __shared__ double wt[kTile][kTile + 1];
    __shared__ double mu_s[kTile];
    const int a = block_pair[blockIdx.x], t = pair_task[a];
    const int n = task_n[t], F = task_f[t], tid = threadIdx.x;
    const int i = block_row0[blockIdx.x] + tid;
    const bool live = i < n;                        // (a thread past the segment works on its first row and writes nothing)
    const int row = row_index[task_row_off[t] + (live ? i : 0)];
    const int32_t *fc = feat_col + task_feat_off[t], *fv = feat_val + task_feat_off[t];
    const int64_t per = 1 + (int64_t)F + (int64_t)F * F;
    double lp[DPL_MAX_CLUSTERS];
#pragma unroll
    for (int k = 0; k < DPL_MAX_CLUSTERS; ++k) lp[k] = 0.0;
    for (int c = 0; c < n_comp; ++c) {
        const double *pc = par + pair_par_off[a] + c * per, *mu = pc + 1, *W = pc + 1 + F;
        double q = 0.0;
        for (int i0 = 0; i0 < F; i0 += kTile) {
            double y[kTile];
#pragma unroll
            for (int ii = 0; ii < kTile; ++ii) y[ii] = 0.0;
            for (int j0 = 0; j0 <= i0; j0 += kTile) {           // (the tiles above the diagonal hold only zeros)
                __syncthreads();
                for (int e = tid; e < kTile * kTile; e += kThreads) {
                    const int ii = e >> 5, jj = e & (kTile - 1);
                    wt[ii][jj] = (i0 + ii < F && j0 + jj < F) ? W[(int64_t)(i0 + ii) * F + j0 + jj] : 0.0;
                }
                if (tid < kTile) mu_s[tid] = j0 + tid < F ? mu[j0 + tid] : 0.0;
                __syncthreads();
                const int jn = min(kTile, F - j0);
                for (int jj = 0; jj < jn; ++jj) {
                    const double d = features.feature(x, n_rows, row, fc[j0 + jj], fv[j0 + jj]) - mu_s[jj];
#pragma unroll
                    for (int ii = 0; ii < kTile; ++ii) y[ii] += wt[ii][jj] * d;
                }
            }
#pragma unroll
            for (int ii = 0; ii < kTile; ++ii) q += y[ii] * y[ii];     // (rows of the tile past F are 0.0)
        }
        const double v = pc[0] + (-0.5 * q);
#pragma unroll
        for (int k = 0; k < DPL_MAX_CLUSTERS; ++k) lp[k] = (k == c) ? v : lp[k];
    }
    if (!live) return;
    double m = lp[0];
    int arg = 0;
#pragma unroll
    for (int k = 1; k < DPL_MAX_CLUSTERS; ++k)
        if (k < n_comp && lp[k] > m) {
            m = lp[k];
            arg = k;
        }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < DPL_MAX_CLUSTERS; ++k)
        if (k < n_comp) s += exp(lp[k] - m);
    const double l = m + log(s);
    const int64_t at = (int64_t)pair_init[a] * n_lab + task_lab_off[t] + i;
    labels[at] = (uint8_t)arg;
    lse[at] = l;
#pragma unroll
    for (int k = 0; k < DPL_MAX_CLUSTERS; ++k)
        if (k < n_comp) resp[at * n_comp + k] = exp(lp[k] - l);
}

__global__ __launch_bounds__(kThreads) void gmm_lse_sum_kernel(
    const int32_t *__restrict__ task_n, const int64_t *__restrict__ task_lab_off, const int32_t *__restrict__ pair_task,
    const int32_t *__restrict__ pair_init, const double *__restrict__ lse, int64_t n_lab, double *__restrict__ lse_sum) {
    __shared__ double part[kThreads];
    const int a = blockIdx.x, t = pair_task[a], n = task_n[t];
    const double *v = lse + (int64_t)pair_init[a] * n_lab + task_lab_off[t];
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += kThreads) s += v[r];
    const double total = sum_in_order(part, s);
    if (threadIdx.x == 0) lse_sum[a] = total;
}

// ---- weighted moments about the pivot: units and groups as in dpl_rdc_gram -------------------------------------------------
template <class Features, bool kMfma>
__global__ __launch_bounds__(kThreads) void gmm_mstats_partial_kernel(
    const typename Features::value *__restrict__ x, int64_t n_rows, const int32_t *__restrict__ row_index, Features features,
    const int64_t *__restrict__ task_row_off, const int64_t *__restrict__ task_lab_off,
    const int32_t *__restrict__ task_feat_off, const int32_t *__restrict__ task_f, const int32_t *__restrict__ feat_col,
    const int32_t *__restrict__ feat_val, const int32_t *__restrict__ pair_task, const int32_t *__restrict__ pair_init,
    const int64_t *__restrict__ pair_par_off, const int32_t *__restrict__ unit_pair, const int32_t *__restrict__ unit_comp,
    const int32_t *__restrict__ unit_i0, const int32_t *__restrict__ unit_j0, const int32_t *__restrict__ unit_row0,
    const int32_t *__restrict__ unit_rows, int n_comp, const double *__restrict__ par, const double *__restrict__ resp,
    int64_t n_lab, double *__restrict__ partial) {
    __shared__ double phi[2][kTile][kTile + 1];
    __shared__ double wrow[kTile];
    const int64_t u = blockIdx.x;
    const int a = unit_pair[u], c = unit_comp[u], i0 = unit_i0[u], j0 = unit_j0[u], r0 = unit_row0[u], nr = unit_rows[u];
    const int t = pair_task[a], F = task_f[t], tid = threadIdx.x;
    const int32_t *rows = row_index + task_row_off[t] + r0;
    const int32_t *fc = feat_col + task_feat_off[t], *fv = feat_val + task_feat_off[t];
    const double *piv = par + pair_par_off[a] + c * (1 + (int64_t)F + (int64_t)F * F) + 1;
    const double *w = resp + ((int64_t)pair_init[a] * n_lab + task_lab_off[t] + r0) * n_comp + c;
    dpl_detail::GramTile<kMfma> tile;
    double ws = 0.0;
    for (int rs = 0; rs < nr; rs += kTile) {        // (nr is block-uniform: every thread takes every trip)
        for (int e = tid; e < 2 * kTile * kTile; e += kThreads) {
            const int side = e >> 10, rr = (e >> 5) & (kTile - 1), fl = e & (kTile - 1);
            const int f = (side ? j0 : i0) + fl;
            double val = 0.0;
            if (rs + rr < nr && f < F) {
                const double d = features.feature(x, n_rows, rows[rs + rr], fc[f], fv[f]) - piv[f];
                val = side ? d : w[(int64_t)(rs + rr) * n_comp] * d;
            }
            phi[side][rr][fl] = val;
        }
        if (tid < kTile) wrow[tid] = rs + tid < nr ? w[(int64_t)(rs + tid) * n_comp] : 0.0;
        __syncthreads();
        tile.step(phi[0], phi[1]);
        if (tid == kTile)
            for (int rr = 0; rr < kTile; ++rr) ws += wrow[rr];
        __syncthreads();
    }
    double *out = partial + u * DPL_GMM_PARTIAL;
    tile.store(out);
    if (tid >= kTile && tid < kTile + DPL_GMM_PARTIAL - DPL_GRAM_PARTIAL) out[DPL_GRAM_PARTIAL + tid - kTile] = tid == kTile ? ws : 0.0;
}

__global__ __launch_bounds__(kThreads) void gmm_mstats_reduce_kernel(
    const int32_t *__restrict__ task_f, const int32_t *__restrict__ pair_task, const int64_t *__restrict__ pair_stat_off,
    const int32_t *__restrict__ unit_pair, const int32_t *__restrict__ unit_comp, const int32_t *__restrict__ unit_i0,
    const int32_t *__restrict__ unit_j0, const int32_t *__restrict__ group_unit0, const int32_t *__restrict__ group_units,
    const double *__restrict__ partial, double *__restrict__ stats) {
    const int64_t u0 = group_unit0[blockIdx.x];
    const int units = group_units[blockIdx.x];
    const int a = unit_pair[u0], c = unit_comp[u0], i0 = unit_i0[u0], j0 = unit_j0[u0], F = task_f[pair_task[a]];
    double *out = stats + pair_stat_off[a] + c * (1 + (int64_t)F + (int64_t)F * F);
    double *s = out + 1, *M = out + 1 + F;
    for (int e = threadIdx.x; e <= DPL_GRAM_PARTIAL; e += kThreads) {
        const double total = dpl_detail::group_total(partial, DPL_GMM_PARTIAL, u0, units, e);
        if (e < kTile * kTile) {
            const int f = i0 + (e >> 5), g = j0 + (e & (kTile - 1));     // f: the weighted factor
            if (f < F && g < F) {
                M[(int64_t)g * F + f] = total;
                if (i0 != j0) M[(int64_t)f * F + g] = total;
            }
        } else if (e < DPL_GRAM_PARTIAL) {
            const int f = i0 + e - kTile * kTile;
            if (i0 == j0 && f < F) s[f] = total;
        } else if (i0 == 0 && j0 == 0) {
            out[0] = total;
        }
    }
}

bool gmm_ok(const void *const *pointers, int n_pointers, int64_t n_pairs, int n_comp, int64_t n_lab, const char *who) {
    for (int k = 0; k < n_pointers; ++k)
        if (pointers[k] == nullptr) {
            set_error("%s: null argument", who);
            return false;
        }
    if (n_pairs < 1 || n_pairs > kMaxGrid || n_comp < 1 || n_comp > DPL_MAX_CLUSTERS || n_lab < 1) {
        set_error("%s: n_pairs = %lld, n_comp = %d (<= %d), n_lab = %lld out of domain", who, (long long)n_pairs, n_comp,
                  DPL_MAX_CLUSTERS, (long long)n_lab);
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

int dpl_gmm_estep(const void *x, int is_float, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                  const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_lab_off,
                  const int32_t *task_feat_off, const int32_t *task_f, const int32_t *feat_col, const int32_t *feat_val,
                  const int32_t *pair_task, const int32_t *pair_init, const int64_t *pair_par_off, int64_t n_pairs,
                  const int32_t *block_pair, const int32_t *block_row0, int64_t n_blocks, int n_init, int n_comp,
                  const double *par, double *resp, uint8_t *labels, double *lse, int64_t n_lab, double *lse_sum,
                  void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_gmm_estep")) return DPL_EINVAL;
    const void *pointers[] = {task_row_off, task_n, task_lab_off, task_feat_off, task_f, feat_col, feat_val, pair_task, pair_init,
                              pair_par_off, block_pair, block_row0, par, resp, labels, lse, lse_sum};
    if (!gmm_ok(pointers, sizeof(pointers) / sizeof(pointers[0]), n_pairs, n_comp, n_lab, "dpl_gmm_estep")) return DPL_EINVAL;
    DPL_REQUIRE(n_blocks >= 1 && n_blocks <= kMaxGrid && n_init >= 1, "dpl_gmm_estep: n_blocks = %lld, n_init = %d out of domain",
                (long long)n_blocks, n_init);
    if (is_float)
        DPL_LAUNCH("dpl_gmm_estep (float32)", gmm_estep_kernel<FloatFeatures>, dim3((unsigned)n_blocks), dim3(kThreads), 0,
                   (hipStream_t)stream, (const float *)x, n_rows, row_index, FloatFeatures{}, task_row_off, task_n, task_lab_off,
                   task_feat_off, task_f, feat_col, feat_val, pair_task, pair_init, pair_par_off, block_pair, block_row0, n_comp,
                   par, resp, labels, lse, n_lab);
    else
        DPL_LAUNCH("dpl_gmm_estep (uint8)", gmm_estep_kernel<OneHotFeatures>, dim3((unsigned)n_blocks), dim3(kThreads), 0,
                   (hipStream_t)stream, (const uint8_t *)x, n_rows, row_index, OneHotFeatures{}, task_row_off, task_n,
                   task_lab_off, task_feat_off, task_f, feat_col, feat_val, pair_task, pair_init, pair_par_off, block_pair,
                   block_row0, n_comp, par, resp, labels, lse, n_lab);
    DPL_LAUNCH("dpl_gmm_estep (sum)", gmm_lse_sum_kernel, dim3((unsigned)n_pairs), dim3(kThreads), 0, (hipStream_t)stream, task_n,
               task_lab_off, pair_task, pair_init, lse, n_lab, lse_sum);
    return DPL_OK;
}

#define DPL_GMM_MSTATS_LAUNCH(FEATURES, TYPE, MFMA, NAME)                                                                       \
    DPL_LAUNCH(NAME, (gmm_mstats_partial_kernel<FEATURES, MFMA>), dim3((unsigned)n_units), dim3(kThreads), 0,                   \
               (hipStream_t)stream, (const TYPE *)x, n_rows, row_index, FEATURES{}, task_row_off, task_lab_off, task_feat_off,  \
               task_f, feat_col, feat_val, pair_task, pair_init, pair_par_off, unit_pair, unit_comp, unit_i0, unit_j0,          \
               unit_row0, unit_rows, n_comp, par, resp, n_lab, partial)

int dpl_gmm_mstats(const void *x, int is_float, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                   const int64_t *task_row_off, const int32_t *task_n, const int64_t *task_lab_off,
                   const int32_t *task_feat_off, const int32_t *task_f, const int32_t *feat_col, const int32_t *feat_val,
                   const int32_t *pair_task, const int32_t *pair_init, const int64_t *pair_par_off,
                   const int64_t *pair_stat_off, int64_t n_pairs, const int32_t *unit_pair, const int32_t *unit_comp,
                   const int32_t *unit_i0, const int32_t *unit_j0, const int32_t *unit_row0, const int32_t *unit_rows,
                   int64_t n_units, const int32_t *group_unit0, const int32_t *group_units, int64_t n_groups, int n_comp,
                   const double *par, const double *resp, int64_t n_lab, int use_mfma, double *partial, double *stats,
                   void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_gmm_mstats")) return DPL_EINVAL;
    const void *pointers[] = {task_row_off, task_n, task_lab_off, task_feat_off, task_f, feat_col, feat_val, pair_task, pair_init,
                              pair_par_off, pair_stat_off, unit_pair, unit_comp, unit_i0, unit_j0, unit_row0, unit_rows,
                              group_unit0, group_units, par, resp, partial, stats};
    if (!gmm_ok(pointers, sizeof(pointers) / sizeof(pointers[0]), n_pairs, n_comp, n_lab, "dpl_gmm_mstats")) return DPL_EINVAL;
    DPL_REQUIRE(n_units >= 1 && n_units <= kMaxGrid && n_groups >= 1 && n_groups <= n_units,
                "dpl_gmm_mstats: n_units = %lld, n_groups = %lld out of domain", (long long)n_units, (long long)n_groups);
    DPL_REQUIRE(n_units * (int64_t)DPL_GMM_PARTIAL * 8 <= (256ll << 20), "dpl_gmm_mstats: %lld units need more than 256 MiB of "
                "partial sums: split the groups over several calls", (long long)n_units);
    if (is_float && use_mfma)
        DPL_GMM_MSTATS_LAUNCH(FloatFeatures, float, true, "dpl_gmm_mstats (float32, matrix core)");
    else if (is_float)
        DPL_GMM_MSTATS_LAUNCH(FloatFeatures, float, false, "dpl_gmm_mstats (float32)");
    else if (use_mfma)
        DPL_GMM_MSTATS_LAUNCH(OneHotFeatures, uint8_t, true, "dpl_gmm_mstats (uint8, matrix core)");
    else
        DPL_GMM_MSTATS_LAUNCH(OneHotFeatures, uint8_t, false, "dpl_gmm_mstats (uint8)");
    DPL_LAUNCH("dpl_gmm_mstats (reduce)", gmm_mstats_reduce_kernel, dim3((unsigned)n_groups), dim3(kThreads), 0,
               (hipStream_t)stream, task_f, pair_task, pair_stat_off, unit_pair, unit_comp, unit_i0, unit_j0, group_unit0,
               group_units, partial, stats);
    return DPL_OK;
}

}  // extern "C"
