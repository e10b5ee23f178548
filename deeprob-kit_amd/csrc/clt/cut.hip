// libdeeprob_clt.so, the scored cutset learners' part (the dpc_cut_* entry points of include/deeprob_clt.h).
//
// learn_cnet_bd / learn_cnet_bic try k candidate cuts per open node and need, for every candidate, the co-occurrence
// counts of the node's rows on each side of the cut.  The side x_c = 1 is a three-way AND + popcount over the planes the
// generation has already packed; the side x_c = 0 is the task's own counts minus it.  cut_pair_counts_kernel is
// seg_pair_counts_kernel of cnet.hip with the entry on grid.z: the words of the cut plane are ANDed into the j operand
// while the step is staged, so the popcount loop is the one of the unconditioned counts.
#include "clt_common.h"

namespace {

using dpc_detail::kMaxGridX;
using dpc_detail::kMaxGridZ;
using dpc_detail::kPairThreads;
using dpc_detail::kPairTile;
using dpc_detail::kPairWords;

typedef unsigned long long u64;

// The rows of the LDS tiles are padded to kPairWords + 1 words as in cnet.hip: the 16 rows a half-wave reads then lie
// 2 banks apart (66 dwords a row, 64 banks for a 64-bit read), and the lanes that share a row read one address.
__global__ __launch_bounds__(kPairThreads) void cut_pair_counts_kernel(const u64 *__restrict__ planes, int64_t n_words,
                                                                      int d, const int32_t *__restrict__ word_off,
                                                                      int n_tasks, const int32_t *__restrict__ entry_task,
                                                                      const int32_t *__restrict__ entry_col,
                                                                      int32_t *__restrict__ ones1) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;            // the mirror image is written by tile (tj, ti)
    __shared__ u64 pi[kPairTile][kPairWords + 1], pj[kPairTile][kPairWords + 1];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int task = entry_task[blockIdx.z], c = entry_col[blockIdx.z];
    // an entry that names no task or no column of the generation counts nothing (and reads nothing through its numbers)
    const bool named = task >= 0 && task < n_tasks && c >= 0 && c < d;
    const int64_t w_begin = named ? word_off[task] : 0, w_end = named ? word_off[task + 1] : 0;
    const u64 *cut = planes + (int64_t)(named ? c : 0) * n_words;
    int acc[2][2] = {{0, 0}, {0, 0}};
    for (int64_t w0 = w_begin; w0 < w_end; w0 += kPairWords) {
        // kPairThreads is a multiple of kPairWords: a thread stages the same word of every row it touches
        const int w = t % kPairWords;
        const bool in = w0 + w < w_end;
        const u64 pc = in ? cut[w0 + w] : 0ull;
        for (int e = t; e < kPairTile * kPairWords; e += kPairThreads) {
            const int r = e / kPairWords;
            const int i = ti * kPairTile + r, j = tj * kPairTile + r;
            pi[r][w] = (in && i < d) ? planes[(int64_t)i * n_words + w0 + w] : 0ull;
            pj[r][w] = (in && j < d) ? planes[(int64_t)j * n_words + w0 + w] & pc : 0ull;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kPairWords; ++k) {
            const u64 a0 = pi[ty][k], a1 = pi[ty + 16][k], b0 = pj[tx][k], b1 = pj[tx + 16][k];
            acc[0][0] += __popcll(a0 & b0);
            acc[0][1] += __popcll(a0 & b1);
            acc[1][0] += __popcll(a1 & b0);
            acc[1][1] += __popcll(a1 & b1);
        }
        __syncthreads();
    }
    int32_t *out = ones1 + (int64_t)blockIdx.z * d * d;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            const int i = ti * kPairTile + ty + 16 * a, j = tj * kPairTile + tx + 16 * b;
            if (i < d && j < d) {
                out[(int64_t)i * d + j] = acc[a][b];
                out[(int64_t)j * d + i] = acc[a][b];
            }
        }
}

static_assert(kPairThreads % kPairWords == 0, "a thread stages one word column");

}  // namespace

extern "C" {

int dpc_cut_pair_counts(const uint64_t *planes, int64_t n_words, int d, const int32_t *word_off, int n_tasks,
                        const int32_t *entry_task, const int32_t *entry_col, int n_entries, int32_t *ones1, void *stream) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "dpc_cut_pair_counts: d = %d is outside 1..%d", d, DPC_MAX_D);
    DPC_REQUIRE(n_tasks >= 1, "dpc_cut_pair_counts: n_tasks = %d is not positive", n_tasks);
    DPC_REQUIRE(n_entries >= 1 && n_entries <= kMaxGridZ, "dpc_cut_pair_counts: n_entries = %d is outside 1..%d", n_entries,
                kMaxGridZ);
    DPC_REQUIRE(n_words >= 0 && n_words <= kMaxGridX, "dpc_cut_pair_counts: n_words = %lld is out of domain",
                (long long)n_words);
    DPC_REQUIRE((planes || n_words == 0) && word_off && entry_task && entry_col && ones1, "dpc_cut_pair_counts: null pointer");
    const unsigned nt = (unsigned)((d + kPairTile - 1) / kPairTile);
    DPC_LAUNCH("dpc_cut_pair_counts", cut_pair_counts_kernel, dim3(nt, nt, (unsigned)n_entries), dim3(kPairThreads), 0,
               (hipStream_t)stream, (const u64 *)planes, n_words, d, word_off, n_tasks, entry_task, entry_col, ones1);
    return DPC_OK;
}

}  // extern "C"
