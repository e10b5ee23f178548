// libdeeprob_clt.so: mixtures of Chow-Liu trees (include/deeprob_clt.h, last section): the likelihoods and
// responsibilities of a batch under all components, and the weighted sufficient statistics of tied-CPT batch EM.  Built
// with -ffp-contract=off like clt.hip: every expression is evaluated operation by operation in the order the header states.
//
// Layout of the work.  Likelihood: one thread per (batch position, component), grid.y = the component, so that a batch of
// a few thousand rows still fills the device; the thread runs tree_log_likelihood of clt_common.h, THE function of
// dpc_clt_log_likelihood, on the row's column-major codes (stride b) with its state in `work` (stride nb).  A second
// launch, one thread per position, mixes the components' values in float32.  Statistics: a work-group owns one chunk of
// DPC_MIX_CHUNK positions and kStatCols columns, for ALL components: thread l owns the positions l, l + 256, ... of the
// chunk (partial l of the header's order), reads their codes of the tile's columns once and keeps them as bits; then per
// component it reads the codes of the tile's PARENT columns (they differ per component, so these bytes are read again for
// every component: K + 1 code reads per row and column in all), accumulates its 1 + 2 kStatCols partials in registers and
// the work-group adds the 256 partials of every output in order of l through LDS.  A last launch adds the chunk sums in
// chunk order.  No atomics; no work-group waits on another.
// How the codes are read: lane l reads byte source_row(l) of a column.  Without a row index that is 64 consecutive bytes per
// wave.  WITH one -- every EM iteration, whose batch is a random draw -- each read is a scattered single byte, and the tile is
// not staged through LDS: the bytes a thread needs are its own rows' alone, so LDS would add a copy without sharing anything;
// gathering the batch's codes into a contiguous buffer first (one more launch, nb * D bytes) is the way to make these reads
// coalesced and has not been built (DESIGN.md 15.1 has the measured cost as it is).
#include "clt_common.h"

namespace {

using dpc_detail::kMaxGridX;
using dpc_detail::Leaf;

constexpr int kRowThreads = 64;     // batch positions per work-group of the likelihood kernels: one wave, as in clt.hip
constexpr int kStatThreads = 256;   // the interleaved partials of a chunk
constexpr int kStatRows = DPC_MIX_CHUNK / kStatThreads;     // positions of a chunk per thread
constexpr int kStatCols = 8;        // columns per work-group
constexpr int kStatOut = 1 + 2 * kStatCols;
static_assert(DPC_MIX_CHUNK % kStatThreads == 0 && kStatOut <= 64, "one wave adds a work-group's partials");

struct MixArgs {
    const uint8_t *codes;
    int64_t b;
    int d;
    const int32_t *rows;
    int64_t nb;
    int n_comp;
    const int32_t *bfs, *parent;
    const float *params;
    const int32_t *child_off, *child_idx;
    const float *logw;
    float *work, *comp_ll, *ll, *resp;
};

// the row of `codes` behind batch position i, -1 if the index names none
__device__ __forceinline__ int64_t source_row(const int32_t *rows, int64_t i, int64_t b) {
    const int64_t s = rows ? (int64_t)rows[i] : i;
    return (s >= 0 && s < b) ? s : -1;
}

__global__ __launch_bounds__(kRowThreads) void mix_components_kernel(const MixArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (i >= a.nb) return;
    const int k = blockIdx.y;
    const int64_t D = a.d;
    const int64_t s = source_row(a.rows, i, a.b);
    float value = NAN;
    if (s >= 0) {
        const Leaf f = {a.d, nullptr, a.bfs + k * D, a.parent + k * D, a.child_off + k * (D + 1), a.child_idx + k * (D - 1),
                        a.params + k * D * 4};
        float *t = a.work ? a.work + (int64_t)k * 2 * D * a.nb + i : nullptr;
        value = dpc_detail::tree_log_likelihood(f, a.codes + s, a.b, t, a.nb);
    }
    a.comp_ll[i * a.n_comp + k] = value;
}

__global__ __launch_bounds__(kRowThreads) void mix_rows_kernel(const MixArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
    if (i >= a.nb) return;
    const int K = a.n_comp;
    const float *c = a.comp_ll + i * K;
    float *resp = a.resp + i * K;
    float top = a.logw[0] + c[0];
    bool bad = top != top;
    for (int k = 1; k < K; ++k) {
        const float ak = a.logw[k] + c[k];
        bad |= ak != ak;
        top = fmaxf(top, ak);
    }
    if (bad) {      // (a position whose row index names no row, or tables that hold NaN)
        a.ll[i] = NAN;
        for (int k = 0; k < K; ++k) resp[k] = NAN;
        return;
    }
    if (top == -INFINITY) {
        a.ll[i] = -INFINITY;
        for (int k = 0; k < K; ++k) resp[k] = 0.f;
        return;
    }
    float sum = 0.f;
    for (int k = 0; k < K; ++k) sum += expf((a.logw[k] + c[k]) - top);
    const float log_sum = logf(sum);
    a.ll[i] = top + log_sum;
    // (not expf(a_k - ll): the rounding of top + log_sum, half an ulp of |ll|, would be a relative error of every resp)
    for (int k = 0; k < K; ++k) resp[k] = expf(((a.logw[k] + c[k]) - top) - log_sum);
}

// part[chunk][k][.]: the chunk sums of the header's order, for the columns j0 .. j0 + kStatCols of the tile blockIdx.y
__global__ __launch_bounds__(kStatThreads) void mix_stats_kernel(const uint8_t *__restrict__ codes, int64_t b, int d,
                                                                 const int32_t *__restrict__ rows, int64_t nb, int n_comp,
                                                                 const float *__restrict__ resp,
                                                                 const int32_t *__restrict__ parent,
                                                                 double *__restrict__ part) {
    // (a row of 257 doubles: the lanes that add the partials of different outputs then read different banks)
    __shared__ double red[kStatOut][kStatThreads + 1];
    const int l = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    const int j0 = blockIdx.y * kStatCols;
    const int64_t width = 1 + 2 * (int64_t)d;

    int64_t pos[kStatRows], src[kStatRows];
    uint32_t bits[kStatRows];
    for (int r = 0; r < kStatRows; ++r) {
        pos[r] = chunk * DPC_MIX_CHUNK + l + r * kStatThreads;
        src[r] = pos[r] < nb ? source_row(rows, pos[r], b) : -1;
        bits[r] = 0;
        if (src[r] >= 0)
            for (int jj = 0; jj < kStatCols; ++jj)
                if (j0 + jj < d && codes[(int64_t)(j0 + jj) * b + src[r]] == 1) bits[r] |= 1u << jj;
    }

    for (int k = 0; k < n_comp; ++k) {
        int pa[kStatCols];
        for (int jj = 0; jj < kStatCols; ++jj) {
            const int p = j0 + jj < d ? parent[(int64_t)k * d + j0 + jj] : -1;
            pa[jj] = (p >= 0 && p < d) ? p : -1;
        }
        double acc[kStatOut];
        for (int o = 0; o < kStatOut; ++o) acc[o] = 0.0;
        for (int r = 0; r < kStatRows; ++r) {       // the positions l, l + 256, ... in order
            if (src[r] < 0) continue;
            const double g = (double)resp[pos[r] * n_comp + k];
            acc[0] += g;
            for (int jj = 0; jj < kStatCols; ++jj) {
                const bool x = (bits[r] >> jj) & 1u;
                // (adding 0.0 leaves a sum that started from 0.0 as it is: the terms of the header's sums are g or 0.0)
                acc[1 + jj] += x ? g : 0.0;
                const bool xp = x && pa[jj] >= 0 && codes[(int64_t)pa[jj] * b + src[r]] == 1;
                acc[1 + kStatCols + jj] += xp ? g : 0.0;
            }
        }
        for (int o = 0; o < kStatOut; ++o) red[o][l] = acc[o];
        __syncthreads();
        if (l < kStatOut) {
            double total = red[l][0];
            for (int t = 1; t < kStatThreads; ++t) total += red[l][t];
            double *out = part + (chunk * n_comp + k) * width;
            if (l == 0) {
                if (blockIdx.y == 0) out[0] = total;
            } else {
                const int jj = (l - 1) % kStatCols;
                if (j0 + jj < d) out[(l <= kStatCols ? 1 : 1 + d) + j0 + jj] = total;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kStatThreads) void mix_stats_sum_kernel(const double *__restrict__ part, int64_t n_chunks,
                                                                     int64_t n_out, double *__restrict__ stats) {
    const int64_t e = (int64_t)blockIdx.x * kStatThreads + threadIdx.x;
    if (e >= n_out) return;
    double total = 0.0;
    if (n_chunks > 0) {
        total = part[e];
        for (int64_t c = 1; c < n_chunks; ++c) total += part[c * n_out + e];
    }
    stats[e] = total;
}

int check_batch(const char *what, const void *codes, int64_t b, int d, const int32_t *rows, int64_t nb, int n_comp) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "%s: d = %d is outside 1..%d", what, d, DPC_MAX_D);
    DPC_REQUIRE(n_comp >= 1 && n_comp <= DPC_MIX_MAX_K, "%s: n_comp = %d is outside 1..%d (DPC_MIX_MAX_K)", what, n_comp,
                DPC_MIX_MAX_K);
    DPC_REQUIRE(b >= 0 && b <= kMaxGridX, "%s: b = %lld is out of domain", what, (long long)b);
    DPC_REQUIRE(nb >= 0 && nb <= kMaxGridX, "%s: nb = %lld is out of domain", what, (long long)nb);
    DPC_REQUIRE(rows || nb == b || nb == 0, "%s: nb = %lld differs from b = %lld without a row index", what, (long long)nb, (long long)b);
    DPC_REQUIRE(codes || b == 0, "%s: null pointer (codes)", what);
    return DPC_OK;
}

}  // namespace

extern "C" {

int dpc_mix_log_likelihood(const uint8_t *codes, int64_t b, int d, const int32_t *rows, int64_t nb, int n_comp,
                           const int32_t *bfs, const int32_t *parent, const float *params, const int32_t *child_off,
                           const int32_t *child_idx, const float *logw, float *work, float *comp_ll, float *ll,
                           float *resp, void *stream) {
    const char *what = "dpc_mix_log_likelihood";
    if (int rc = check_batch(what, codes, b, d, rows, nb, n_comp)) return rc;
    DPC_REQUIRE(bfs && parent && params && child_off && logw, "%s: null pointer", what);
    DPC_REQUIRE(child_idx || d == 1, "%s: null pointer (child_idx)", what);
    if (nb == 0) return DPC_OK;
    DPC_REQUIRE(comp_ll && ll && resp, "%s: null pointer", what);      // (work may be null: the header)
    const MixArgs a = {codes, b, d, rows, nb, n_comp, bfs, parent, params, child_off, child_idx, logw, work, comp_ll, ll, resp};
    const unsigned grid = (unsigned)((nb + kRowThreads - 1) / kRowThreads);
    DPC_LAUNCH(what, mix_components_kernel, dim3(grid, (unsigned)n_comp), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    DPC_LAUNCH(what, mix_rows_kernel, dim3(grid), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    return DPC_OK;
}

int dpc_mix_em_stats(const uint8_t *codes, int64_t b, int d, const int32_t *rows, int64_t nb, int n_comp,
                     const float *resp, const int32_t *parent, double *part, double *stats, void *stream) {
    const char *what = "dpc_mix_em_stats";
    if (int rc = check_batch(what, codes, b, d, rows, nb, n_comp)) return rc;
    DPC_REQUIRE(parent && stats, "%s: null pointer", what);
    DPC_REQUIRE((resp && part) || nb == 0, "%s: null pointer", what);
    const int64_t n_chunks = (nb + DPC_MIX_CHUNK - 1) / DPC_MIX_CHUNK;
    const int64_t n_out = (int64_t)n_comp * (1 + 2 * (int64_t)d);
    if (n_chunks > 0)
        DPC_LAUNCH(what, mix_stats_kernel, dim3((unsigned)n_chunks, (unsigned)((d + kStatCols - 1) / kStatCols)),
                   dim3(kStatThreads), 0, (hipStream_t)stream, codes, b, d, rows, nb, n_comp, resp, parent, part);
    DPC_LAUNCH(what, mix_stats_sum_kernel, dim3((unsigned)((n_out + kStatThreads - 1) / kStatThreads)), dim3(kStatThreads), 0,
               (hipStream_t)stream, (const double *)part, n_chunks, n_out, stats);
    return DPC_OK;
}

}  // extern "C"
