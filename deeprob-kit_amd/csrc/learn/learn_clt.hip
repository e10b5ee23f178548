// libdeeprob_learn.so, the statistic of Chow-Liu tree leaves (dpl_pair_ones of include/deeprob_learn.h): the co-occurrence
// counts of every leaf task of one generation, on the learner's own layout -- uint8, column major, rows through the
// row-index array, a subset of the columns per task.
//
// The scheme is the one of dpc_cnet_gather_pack / dpc_cnet_pair_counts (csrc/clt/cnet.hip) with the two steps in one
// kernel and the bit planes in LDS only: a wave gathers 64 rows of a column and `__ballot(x == 1)` is that column's 64-bit
// word; 16 such words (1024 rows) of the 64 columns of two column tiles make one pass; every thread then owns a 4 x 4
// patch of the 64 x 64 pairs and adds popcount(a & b) over the pass's words.  A UNIT is one tile pair ti <= tj of one task
// over one chunk of its rows; the planes of a task of any width are thereby tiled over columns, and a long segment is
// spread over several work-groups.  Units of one task meet in global memory by integer atomics -- the order of integer
// additions is free --, so the entry zeroes the output with a kernel of its own first.
#include "learn_common.h"

namespace {

using dpl_detail::common_ok;
using dpl_detail::kMaxGrid;
using dpl_detail::kThreads;

typedef unsigned long long u64;
constexpr int kTile = DPL_PAIR_TILE;    // columns of a tile
constexpr int kWords = 16;              // 64-row words of a pass
static_assert(kTile == 64 && kThreads == 256, "a lane per column of a tile, a 4 x 4 patch of pairs per thread");

__global__ __launch_bounds__(kThreads) void zero_kernel(int32_t *__restrict__ out, int64_t n) {
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) out[e] = 0;
}

// planes[c][w] <- the word of rows [(w0 + w) * 64, + 64) of the unit for column c of the tile that starts at `first`;
// columns past the task's m, rows past the unit's n and indices outside the data give 0 bits.  Wave `wave` makes the
// words wave, wave + 4, ...; every lane stores one word, so [0, kTile) x [0, nw) is written.
__device__ __forceinline__ void pack_tile(u64 (*planes)[kWords + 1], const uint8_t *__restrict__ x, int64_t n_rows,
                                          int n_cols, const int32_t *__restrict__ cols, int first, int m,
                                          const int32_t *__restrict__ rows, int n, int w0, int nw) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mc = min(kTile, m - first);
    for (int w = wave; w < nw; w += kThreads / 64) {
        const int r = (w0 + w) * 64 + lane;
        int64_t row = (r < n) ? (int64_t)rows[r] : -1;
        if (row >= n_rows) row = -1;
        u64 mine = 0;
        for (int c = 0; c < mc; ++c) {
            const int col = cols[first + c];    // (wave uniform)
            const bool one = row >= 0 && col >= 0 && col < n_cols && x[(int64_t)col * n_rows + row] == 1;
            const u64 mask = __ballot(one);
            if (lane == c) mine = mask;
        }
        planes[lane][w] = mine;
    }
}

__global__ __launch_bounds__(kThreads) void pair_ones_kernel(
    const uint8_t *__restrict__ x, int64_t n_rows, int n_cols, const int32_t *__restrict__ row_index,
    const int32_t *__restrict__ blk_col, const int64_t *__restrict__ blk_col_off, const int32_t *__restrict__ blk_m,
    const int64_t *__restrict__ blk_row_off, const int32_t *__restrict__ blk_n, const int64_t *__restrict__ blk_out_off,
    const int32_t *__restrict__ unit_blk, const int32_t *__restrict__ unit_ti, const int32_t *__restrict__ unit_tj,
    const int32_t *__restrict__ unit_row0, int row_chunk, int32_t *__restrict__ ones) {
    __shared__ u64 pi[kTile][kWords + 1], pj[kTile][kWords + 1];
    const int64_t u = blockIdx.x;
    const int b = unit_blk[u], ti = unit_ti[u], tj = unit_tj[u], row0 = unit_row0[u];
    const int m = blk_m[b];
    const int n = min(row_chunk, blk_n[b] - row0);      // (the rows of this unit; block uniform, as all of the above)
    const int32_t *cols = blk_col + blk_col_off[b];
    const int32_t *rows = row_index + blk_row_off[b] + row0;
    const bool square = ti == tj;
    const u64(*pb)[kWords + 1] = square ? pi : pj;
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    int acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0;
    const int n_words = (n + 63) / 64;
    for (int w0 = 0; w0 < n_words; w0 += kWords) {
        const int nw = min(kWords, n_words - w0);
        pack_tile(pi, x, n_rows, n_cols, cols, ti * kTile, m, rows, n, w0, nw);
        if (!square) pack_tile(pj, x, n_rows, n_cols, cols, tj * kTile, m, rows, n, w0, nw);
        __syncthreads();
        for (int w = 0; w < nw; ++w) {
            u64 va[4], vb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) va[a] = pi[ty + 16 * a][w];
#pragma unroll
            for (int c = 0; c < 4; ++c) vb[c] = pb[tx + 16 * c][w];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] += __popcll(va[a] & vb[c]);
        }
        __syncthreads();
    }
    int32_t *out = ones + blk_out_off[b];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = ti * kTile + ty + 16 * a, j = tj * kTile + tx + 16 * c;
            if (i < m && j < m && acc[a][c] != 0) {
                atomicAdd(&out[(int64_t)i * m + j], acc[a][c]);
                if (!square) atomicAdd(&out[(int64_t)j * m + i], acc[a][c]);     // (a square tile holds both (i, j) and (j, i))
            }
        }
}

}  // namespace

extern "C" int dpl_pair_ones(const uint8_t *x, int64_t n_rows, int n_cols, const int32_t *row_index, int64_t n_index,
                             const int32_t *blk_col, const int64_t *blk_col_off, const int32_t *blk_m,
                             const int64_t *blk_row_off, const int32_t *blk_n, const int64_t *blk_out_off, int64_t n_blocks,
                             const int32_t *unit_blk, const int32_t *unit_ti, const int32_t *unit_tj,
                             const int32_t *unit_row0, int64_t n_units, int row_chunk, int32_t *ones, int64_t n_ones,
                             void *stream) {
    if (!common_ok(x, n_rows, n_cols, row_index, n_index, "dpl_pair_ones")) return DPL_EINVAL;
    DPL_REQUIRE(blk_col && blk_col_off && blk_m && blk_row_off && blk_n && blk_out_off && unit_blk && unit_ti && unit_tj &&
                    unit_row0 && ones, "dpl_pair_ones: null argument");
    DPL_REQUIRE(n_blocks >= 1 && n_units >= 1 && n_units <= kMaxGrid && n_ones >= 1 && row_chunk >= 1,
                "dpl_pair_ones: n_blocks = %lld, n_units = %lld, n_ones = %lld, row_chunk = %d out of domain", (long long)n_blocks,
                (long long)n_units, (long long)n_ones, row_chunk);
    const int64_t zero_blocks = (n_ones + kThreads - 1) / kThreads;
    DPL_LAUNCH("dpl_pair_ones", zero_kernel, dim3((unsigned)(zero_blocks < 4096 ? zero_blocks : 4096)), dim3(kThreads), 0,
               (hipStream_t)stream, ones, n_ones);
    DPL_LAUNCH("dpl_pair_ones", pair_ones_kernel, dim3((unsigned)n_units), dim3(kThreads), 0, (hipStream_t)stream, x, n_rows,
               n_cols, row_index, blk_col, blk_col_off, blk_m, blk_row_off, blk_n, blk_out_off, unit_blk, unit_ti, unit_tj,
               unit_row0, row_chunk, ones);
    return DPL_OK;
}
