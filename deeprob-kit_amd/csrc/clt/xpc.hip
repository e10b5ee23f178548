// libdeeprob_clt.so, the XPC learners' part (the dpc_xpc_* entry points of include/deeprob_clt.h).
//
// An XPC splits a row segment by a CONJUNCTION of conj_len binary variables: a row's code is the conj_len bits it holds in
// the task's conjunction columns, and the segment goes 2^conj_len ways at most.  Both entries read the bit planes of the
// WHOLE training matrix (dpc_pack_bits) through the row index -- conj_len words per 64 consecutive rows, no gather-pack per
// split -- and cut a task's segment into chunks of DPC_XPC_CHUNK rows, one work-group each (the chunk's task is found by
// bisection of chunk_off, as gather_pack_kernel of cnet.hip finds a word's task).
//
//   code_hist_kernel    one work-group per chunk: the histogram of the chunk's codes in LDS (integer adds), stored whole;
//   hist_sum_kernel     one work-group per task, thread = code: the serial sum of the task's chunk histograms;
//   partition_kernel    one work-group per chunk: thread = code sums the histograms of the task's chunks IN FRONT of this
//                       one, the sums are folded per child into the chunk's first output position of every child, and
//                       the rows of the chunk are ranked among the rows of their child 64 at a time: the lanes of a wave
//                       that hold the same child are found with one ballot per bit of the child number, the rank inside
//                       the wave is a popcount of that mask below the lane, and the 16 waves' worth of a chunk are
//                       chained through a [16][2^conj_len] table of counts in LDS.  No global atomics, no scan through
//                       memory, no work-group waits on another; the split is stable by construction.
#include "clt_common.h"

namespace {

using dpc_detail::kMaxGridX;

typedef unsigned long long u64;
constexpr int kThreads = 256;
constexpr int kChunk = DPC_XPC_CHUNK;
constexpr int kMaxCodes = 1 << DPC_XPC_MAX_CONJ;
constexpr int kGroups = kChunk / 64;                    // 64-row groups of a chunk
constexpr int kGroupsPerWave = kGroups / (kThreads / 64);
static_assert(kMaxCodes == kThreads, "a thread per code");
static_assert(kChunk % kThreads == 0 && kGroups % (kThreads / 64) == 0, "whole waves of rows");

struct Chunk {
    int task;
    int64_t first, end;     // positions in `rows` of the chunk's rows
    int chunk0;             // the first chunk of the task
};

__device__ __forceinline__ Chunk chunk_of(const int32_t *__restrict__ seg_off, const int32_t *__restrict__ chunk_off,
                                          int n_tasks, int chunk) {
    int lo = 0, hi = n_tasks - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (chunk_off[mid + 1] <= chunk) lo = mid + 1; else hi = mid;
    }
    const int64_t first = (int64_t)seg_off[lo] + (int64_t)(chunk - chunk_off[lo]) * kChunk;
    const int64_t seg_end = seg_off[lo + 1];
    return {lo, first, first + kChunk < seg_end ? first + kChunk : seg_end, chunk_off[lo]};
}

// the code of training row r; a row outside 0 .. n-1 and a column outside 0 .. d-1 read as zeros
__device__ __forceinline__ int code_of(const u64 *__restrict__ planes, int64_t n_words, int64_t n, int d,
                                       const int32_t *cols, int conj_len, int64_t r) {
    int code = 0;
    if (r < 0 || r >= n) return 0;
    for (int i = 0; i < conj_len; ++i) {
        const int c = cols[i];
        if (c >= 0 && c < d) code |= (int)((planes[(int64_t)c * n_words + (r >> 6)] >> (r & 63)) & 1ull) << i;
    }
    return code;
}

__global__ __launch_bounds__(kThreads) void code_hist_kernel(const u64 *__restrict__ planes, int64_t n_words, int64_t n,
                                                             int d, const int32_t *__restrict__ rows,
                                                             const int32_t *__restrict__ seg_off,
                                                             const int32_t *__restrict__ chunk_off,
                                                             const int32_t *__restrict__ conj_cols, int conj_len,
                                                             int n_tasks, int32_t *__restrict__ chunk_hist) {
    __shared__ int hist[kMaxCodes];
    __shared__ int32_t cols[DPC_XPC_MAX_CONJ];
    const Chunk ch = chunk_of(seg_off, chunk_off, n_tasks, blockIdx.x);
    hist[threadIdx.x] = 0;
    if (threadIdx.x < conj_len) cols[threadIdx.x] = conj_cols[(int64_t)ch.task * conj_len + threadIdx.x];
    __syncthreads();
    for (int64_t p = ch.first + threadIdx.x; p < ch.end; p += kThreads)
        atomicAdd(&hist[code_of(planes, n_words, n, d, cols, conj_len, rows[p])], 1);
    __syncthreads();
    const int n_codes = 1 << conj_len;
    if ((int)threadIdx.x < n_codes) chunk_hist[(int64_t)blockIdx.x * n_codes + threadIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void hist_sum_kernel(const int32_t *__restrict__ chunk_off,
                                                            const int32_t *__restrict__ chunk_hist, int conj_len,
                                                            int32_t *__restrict__ hist) {
    const int t = blockIdx.x, n_codes = 1 << conj_len;
    if ((int)threadIdx.x >= n_codes) return;
    int sum = 0;
    for (int c = chunk_off[t]; c < chunk_off[t + 1]; ++c) sum += chunk_hist[(int64_t)c * n_codes + threadIdx.x];
    hist[(int64_t)t * n_codes + threadIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void xpc_partition_kernel(const u64 *__restrict__ planes, int64_t n_words, int64_t n,
                                                                 int d, const int32_t *__restrict__ rows,
                                                                 const int32_t *__restrict__ seg_off,
                                                                 const int32_t *__restrict__ chunk_off,
                                                                 const int32_t *__restrict__ conj_cols, int conj_len,
                                                                 const int32_t *__restrict__ chunk_hist,
                                                                 const int32_t *__restrict__ child_of_code,
                                                                 const int32_t *__restrict__ out_off, int n_tasks,
                                                                 int32_t *__restrict__ rows_out) {
    __shared__ int child_of[kMaxCodes];         // code -> child
    __shared__ int base[kMaxCodes];             // child -> rows of that child in the chunks in front of this one
    __shared__ int count[kGroups][kMaxCodes];   // [group][child] -> rows, then the group's first output position
    __shared__ int32_t cols[DPC_XPC_MAX_CONJ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_codes = 1 << conj_len;
    const Chunk ch = chunk_of(seg_off, chunk_off, n_tasks, blockIdx.x);

    base[threadIdx.x] = 0;
    for (int g = 0; g < kGroups; ++g) count[g][threadIdx.x] = 0;
    int mine = 0;                               // a child outside 0 .. 2^conj_len - 1 is taken as child 0
    if ((int)threadIdx.x < n_codes) {
        mine = child_of_code[(int64_t)ch.task * n_codes + threadIdx.x];
        if (mine < 0 || mine >= n_codes) mine = 0;
    }
    child_of[threadIdx.x] = mine;
    if (threadIdx.x < conj_len) cols[threadIdx.x] = conj_cols[(int64_t)ch.task * conj_len + threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < n_codes) {
        int before = 0;
        for (int c = ch.chunk0; c < (int)blockIdx.x; ++c) before += chunk_hist[(int64_t)c * n_codes + threadIdx.x];
        if (before) atomicAdd(&base[mine], before);
    }

    // the child of every row of the chunk, its rank among the rows of that child in its group of 64, the group's counts
    int child[kGroupsPerWave], rank[kGroupsPerWave];
    int32_t row[kGroupsPerWave];
    for (int i = 0; i < kGroupsPerWave; ++i) {
        const int g = wave * kGroupsPerWave + i;
        const int64_t p = ch.first + g * 64 + lane;
        const bool in = p < ch.end;
        row[i] = in ? rows[p] : 0;
        child[i] = in ? child_of[code_of(planes, n_words, n, d, cols, conj_len, row[i])] : 0;
        u64 same = __ballot(in);
        for (int b = 0; b < conj_len; ++b) {
            const u64 set = __ballot((child[i] >> b) & 1);
            same &= ((child[i] >> b) & 1) ? set : ~set;
        }
        rank[i] = __popcll(same & ((1ull << lane) - 1ull));
        if (in && rank[i] == 0) count[g][child[i]] = __popcll(same);
        if (!in) child[i] = -1;
    }
    __syncthreads();
    if ((int)threadIdx.x < n_codes) {           // thread = child: counts -> first output positions, group after group
        int at = out_off[(int64_t)ch.task * n_codes + threadIdx.x] + base[threadIdx.x];
        for (int g = 0; g < kGroups; ++g) {
            const int here = count[g][threadIdx.x];
            count[g][threadIdx.x] = at;
            at += here;
        }
    }
    __syncthreads();
    for (int i = 0; i < kGroupsPerWave; ++i)
        if (child[i] >= 0) rows_out[(int64_t)count[wave * kGroupsPerWave + i][child[i]] + rank[i]] = row[i];
}

int check(const char *who, const void *planes, int64_t n_words, int64_t n, int d, int conj_len, int n_tasks, int n_chunks) {
    DPC_REQUIRE(d >= 1 && d <= DPC_MAX_D, "%s: d = %d is outside 1..%d", who, d, DPC_MAX_D);
    DPC_REQUIRE(n >= 1 && n < 2147483648ll, "%s: n = %lld is outside 1..2^31-1", who, (long long)n);
    DPC_REQUIRE(n_words == (n + 63) / 64, "%s: n_words = %lld is not (n + 63) / 64", who, (long long)n_words);
    DPC_REQUIRE(conj_len >= 1 && conj_len <= DPC_XPC_MAX_CONJ, "%s: conj_len = %d is outside 1..%d", who, conj_len,
                DPC_XPC_MAX_CONJ);
    DPC_REQUIRE(n_tasks >= 1 && n_tasks <= kMaxGridX, "%s: n_tasks = %d is not positive", who, n_tasks);
    DPC_REQUIRE(n_chunks >= 0 && n_chunks <= kMaxGridX >> DPC_XPC_MAX_CONJ, "%s: n_chunks = %d is out of domain", who,
                n_chunks);
    DPC_REQUIRE(planes, "%s: null pointer", who);
    return DPC_OK;
}

}  // namespace

extern "C" {

int dpc_xpc_code_counts(const uint64_t *planes, int64_t n_words, int64_t n, int d, const int32_t *rows,
                        const int32_t *seg_off, const int32_t *chunk_off, const int32_t *conj_cols, int conj_len,
                        int n_tasks, int n_chunks, int32_t *chunk_hist, int32_t *hist, void *stream) {
    const int rc = check("dpc_xpc_code_counts", planes, n_words, n, d, conj_len, n_tasks, n_chunks);
    if (rc != DPC_OK) return rc;
    DPC_REQUIRE(rows && seg_off && chunk_off && conj_cols && hist && (chunk_hist || n_chunks == 0),
                "dpc_xpc_code_counts: null pointer");
    if (n_chunks > 0)
        DPC_LAUNCH("dpc_xpc_code_counts", code_hist_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, (hipStream_t)stream,
                   (const u64 *)planes, n_words, n, d, rows, seg_off, chunk_off, conj_cols, conj_len, n_tasks, chunk_hist);
    DPC_LAUNCH("dpc_xpc_code_counts", hist_sum_kernel, dim3((unsigned)n_tasks), dim3(kThreads), 0, (hipStream_t)stream,
               chunk_off, chunk_hist, conj_len, hist);
    return DPC_OK;
}

int dpc_xpc_partition(const uint64_t *planes, int64_t n_words, int64_t n, int d, const int32_t *rows, const int32_t *seg_off,
                      const int32_t *chunk_off, const int32_t *conj_cols, int conj_len, const int32_t *chunk_hist,
                      const int32_t *child_of_code, const int32_t *out_off, int n_tasks, int n_chunks, int32_t *rows_out,
                      void *stream) {
    const int rc = check("dpc_xpc_partition", planes, n_words, n, d, conj_len, n_tasks, n_chunks);
    if (rc != DPC_OK) return rc;
    DPC_REQUIRE(rows && seg_off && chunk_off && conj_cols && child_of_code && out_off, "dpc_xpc_partition: null pointer");
    if (n_chunks == 0) return DPC_OK;
    DPC_REQUIRE(chunk_hist && rows_out, "dpc_xpc_partition: null pointer");
    DPC_LAUNCH("dpc_xpc_partition", xpc_partition_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, (hipStream_t)stream,
               (const u64 *)planes, n_words, n, d, rows, seg_off, chunk_off, conj_cols, conj_len, chunk_hist, child_of_code,
               out_off, n_tasks, rows_out);
    return DPC_OK;
}

}  // extern "C"
