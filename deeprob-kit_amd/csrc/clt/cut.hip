// libdeeprob_clt.so, the scored cutset learners' part (the dpc_cut_* entry points of include/deeprob_clt.h).
//
// learn_cnet_bd / learn_cnet_bic try k candidate cuts per open node and need, for every candidate, the co-occurrence
// counts of the node's rows on each side of the cut.  The side x_c = 1 is a three-way AND + popcount over the planes the
// generation has already packed; the side x_c = 0 is the task's own counts minus it.  cut_pair_counts_kernel is the pair
// tile of clt_common.h (pair_tile<true>, the one definition behind clt.hip's and cnet.hip's counts too) with the entry on
// grid.z: the words of the cut plane are ANDed into the j operand while the step is staged, so the popcount loop is the
// one of the unconditioned counts.
#include "clt_common.h"

namespace {

using dpc_detail::kMaxGridX;
using dpc_detail::kMaxGridZ;
using dpc_detail::kPairThreads;
using dpc_detail::kPairTile;
using dpc_detail::pair_tile;

typedef unsigned long long u64;

__global__ __launch_bounds__(kPairThreads) void cut_pair_counts_kernel(const u64 *__restrict__ planes, int64_t n_words,
                                                                      int d, const int32_t *__restrict__ word_off,
                                                                      int n_tasks, const int32_t *__restrict__ entry_task,
                                                                      const int32_t *__restrict__ entry_col,
                                                                      int32_t *__restrict__ ones1) {
    const int task = entry_task[blockIdx.z], c = entry_col[blockIdx.z];
    // an entry that names no task or no column of the generation counts nothing (and reads nothing through its numbers)
    const bool named = task >= 0 && task < n_tasks && c >= 0 && c < d;
    pair_tile<true>(planes, n_words, d, named ? word_off[task] : 0, named ? word_off[task + 1] : 0,
                    planes + (int64_t)(named ? c : 0) * n_words, ones1 + (int64_t)blockIdx.z * d * d);
}

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
