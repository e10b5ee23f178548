// What the two Gram kernels of libdeeprob_learn.so share (dpl_rdc_gram in learn_cont.hip, dpl_gmm_mstats in learn_gmm.hip):
// the products of two 32-feature tiles held in LDS, 32 rows at a step, on the VALU or on v_mfma_f64_16x16x4_f64, the layout
// of a unit's partial sums and the in-order sum of a group's units.
#pragma once
#include "learn_common.h"

namespace dpl_detail {
constexpr int kTile = DPL_GRAM_TILE;      // features of a tile, and rows of a tile held in LDS at a time
static_assert(kTile == 32 && DPL_GRAM_PARTIAL == kTile * kTile + kTile && kThreads == 256, "2 x 2 products per thread");

typedef double double4_t __attribute__((ext_vector_type(4)));

// The running products of one unit: out[i][j] += sum_rr pi[rr][i] * pj[rr][j] and cs[i] += sum_rr pi[rr][i].
// kMfma: the products of a 32-row step run on v_mfma_f64_16x16x4_f64 -- wave v owns the 16 x 16 quarter (v >> 1, v & 1) of
// the tile pair, A = pi^T and B = pj taken from LDS one f64 per lane (A: feature lane & 15, row lane >> 4 of the
// 4-row block; B likewise), D: column lane & 15, row (lane >> 4) + 4 * register -- else on the VALU, 2 x 2 products per
// thread.  The column sums are added row by row in both.
template <bool kMfma>
struct GramTile {
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, cs = 0.0;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};

    // one 32-row step; the caller's barriers stand around it
    __device__ __forceinline__ void step(const double (*pi)[kTile + 1], const double (*pj)[kTile + 1]) {
        const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
        const int wave = tid >> 6, lane = tid & 63, qi = (wave >> 1) * 16, qj = (wave & 1) * 16;
        if constexpr (kMfma) {
            for (int r4 = 0; r4 < kTile; r4 += 4) {
                const int rr = r4 + (lane >> 4);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pi[rr][qi + (lane & 15)], pj[rr][qj + (lane & 15)], acc, 0, 0, 0);
            }
            if (tid < kTile)
                for (int rr = 0; rr < kTile; ++rr) cs += pi[rr][tid];
        } else {
            for (int rr = 0; rr < kTile; ++rr) {
                const double x0 = pi[rr][ti], x1 = pi[rr][ti + 16], y0 = pj[rr][tj], y1 = pj[rr][tj + 16];
                a00 += x0 * y0;
                a01 += x0 * y1;
                a10 += x1 * y0;
                a11 += x1 * y1;
                if (tid < kTile) cs += pi[rr][tid];
            }
        }
    }

    // out: DPL_GRAM_PARTIAL numbers, the 32 x 32 products (row major) and then the 32 column sums
    __device__ __forceinline__ void store(double *__restrict__ out) const {
        const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
        const int wave = tid >> 6, lane = tid & 63, qi = (wave >> 1) * 16, qj = (wave & 1) * 16;
        if constexpr (kMfma) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) out[(qi + (lane >> 4) + 4 * reg) * kTile + qj + (lane & 15)] = acc[reg];
        } else {
            out[ti * kTile + tj] = a00;
            out[ti * kTile + tj + 16] = a01;
            out[(ti + 16) * kTile + tj] = a10;
            out[(ti + 16) * kTile + tj + 16] = a11;
        }
        if (tid < kTile) out[kTile * kTile + tid] = cs;
    }
};

// element e of the partial sums of the units u0 .. u0 + units, `stride` numbers apart, added in that order
__device__ __forceinline__ double group_total(const double *__restrict__ partial, int64_t stride, int64_t u0, int units, int e) {
    double total = partial[u0 * stride + e];
    for (int c = 1; c < units; ++c) total += partial[(u0 + c) * stride + e];
    return total;
}
}  // namespace dpl_detail
