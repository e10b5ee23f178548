// RAT-SPN fused forward with the leaf layer on the matrix cores (depth 2, unit-scale Gaussian leaves).
//
// reference: RegionGraphLayer.forward + GaussianLayer (deeprob/spn/layers/ratspn.py:87-108, :160-213),
// ProductLayer :272-286, SumLayer :363-378, RootLayer :446-458, chained by RatSpn.forward
// (deeprob/spn/models/ratspn.py:105-122).
//
// With sigma == 1 the leaf sum of region r, channel k is
//     sum_f [f in r] ( x_f mu_rkf - mu_rkf^2/2 - log sqrt(2 pi) )  -  1/2 sum_f [f in r] x_f^2 .
// The first part is a GEMM  P[b, n] = sum_f x[b, f] M[f, n]  over the n = (repetition, region, channel)
// columns, with M[f, n] = mu where variable f belongs to the region of column n and 0 elsewhere (one
// region per repetition holds f: M is 1/4 dense at depth 2).  The second part is common to the channels
// of a region, hence factors out of every sum node above it; every repetition covers each variable once,
// so what reaches the root is -1/2 sum_f x_f^2: one scalar per sample.
//
// The GEMM runs on v_mfma_f32_32x32x16_f16 with both operands split into two f16 halves (x = xh + xl,
// mu = mh + ml, each half carrying 11 significant bits): x mu ~= mh xh + mh xl + ml xh, accumulated in
// fp32; the dropped ml xl term is below 2^-22 |x mu|, i.e. the product keeps fp32 accuracy.  Three f16
// MFMAs cost 3/16 of one fp32 MFMA, so even the dense form of the 1/4-dense matrix is ~5x cheaper than
// the VALU form -- and, unlike it, leaves the kernel bound by the HBM stream of x.
//
// The constants: a chunk of 64 features without marginalised evidence adds its per-column sums of
// -(mu^2/2 + log sqrt(2 pi)) ready-made (prepared table).  In a chunk that holds NaN evidence the NaN
// entries become 0 and the constants of the OBSERVED variables only are accumulated by a second GEMM, a 0/1
// validity indicator against the table of negated constants -- marginalisation is exact in the same form,
// nothing is added and subtracted again, and an all-NaN row comes out as exactly 0 like the reference's.
// Anything the expanded square cannot carry within the 1e-5 bar (+-inf or huge evidence, a sample whose
// sum of squares is large, means beyond kExpandBound, non-unit scales) sends the 32 samples of the wave
// through an exact per-element evaluation (gemm_exact_wave) -- correctness never depends on the hint.
//
// Mapping: a work-group of 4 waves owns 128 samples, a wave 32 of them.  The x tile streams through LDS
// in chunks of 64 features by LDS-DMA (global_load_lds_dwordx4: full 256-byte row segments from HBM, the
// 16-byte pieces XOR-swizzled on the SOURCE side so that the MFMA-shaped ds_read_b128 is conflict free),
// three stages deep, counted vmcnt + raw s_barrier (no drain across the barrier).  The mean-table chunk
// (16 KB of ready-made MFMA A-fragments, L2 resident) rides in the same stages.  The MFMA computes
// P^T = M^T x^T, so a lane ends up holding, for ONE sample, the 16 columns of half a repetition set:
// lane l (sample l & 31, half h = l >> 5) owns regions {2h, 2h+1} of every repetition, evaluates that
// partition's product + sum nodes in registers, swaps the S outputs with lane l ^ 32 and finishes the
// root.  Work-groups are persistent (grid = min(tiles, CUs)); the DMA ring runs across tile boundaries.
#include "common.h"
#include "ratspn_gemm_fused.h"
#include "ratspn_gemm_prep.h"
#include <math.h>
#include <stdlib.h>
#include <algorithm>

namespace dpk {

// ------------------------------------------------------------------------------------------------
// tables, rebuilt from the live parameters (ratspn_gemm_prep.h): one work-group per repetition slot + the softmax rows
// behind them.  This is the stand-alone launch (kPrepBuild / kPrepVerify); the small-batch and 8-channel kernels run the
// same work-groups inside their own launch (kPrepInline).
// ------------------------------------------------------------------------------------------------
template <int I>
__global__ __launch_bounds__(kGemmPrepThreads) void ratspn_gemm_prep_kernel(const GemmPrepArgs a) {
    extern __shared__ int prep_dyn[];
    if (a.mode == kPrepBuild && blockIdx.x == 0) {   // (no launch of this module is in flight: stream order)
        if (threadIdx.x == 0) {
            a.ctl->word = 0ull;
            a.ctl->readers = 0u;
        }
        // (the slice mapping's check, ratspn_gemm_slice.hip SliceVerify: counters that only grow from here)
        unsigned long long *sv = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(a.ctl) + 64);
        for (int i = (int)threadIdx.x; i < kSliceVerifyBytes / 8; i += (int)blockDim.x) sv[i] = 0ull;
        // (8-channel models: the tickets of blocks shared by two work-groups, ratspn_gemm_wide.hip)
        if (a.wx_tick != nullptr)
            for (int i = (int)threadIdx.x; i < kWideSplitBlocks; i += (int)blockDim.x) a.wx_tick[i] = 0u;
    }
    gemm_prep_block<I>(a, (int)blockIdx.x, prep_dyn);
}

// The ring kernel below is kept exactly as round 2 left it, in a namespace of its own with its own argument block and
// its own copy of the upper layers: its hand-balanced schedule (one compute wave per SIMD, LDS-DMA ring, counted waits)
// moved by 3-7 us of 46 when the upper layers were factored into a function shared with the other two mappings, when a
// template flag for the marginalised-evidence variant was threaded through it, and by 0.7 us when three fields were
// appended to its argument block (same-box A/B runs, round 3).  The small-batch kernel (ratspn_gemm_small.hip) and the
// marginalised-evidence variant (ratspn_gemm_nan.hip) share ratspn_gemm_fused.h instead.
namespace ring {

// ------------------------------------------------------------------------------------------------
// main kernel
// ------------------------------------------------------------------------------------------------
struct GemmArgs {
    const float *x;
    int64_t B;
    int D, d, reps, C, NCH, ntiles;
    const uint16_t *mtab, *ctab;
    const float *biasT;   // [2][NT][16] whole-row constants in the accumulator order of a lane
    const float *biasC;   // [NCH][2][NT][16] the same per chunk (tiles with marginalised evidence)
    const int *elig;
    const float *W0;   // [reps*2][S][I*I] linear softmax weights (copied into LDS)
    const float *LW0;  // log-softmax weights (exact fallback of a node, exact evaluation)
    cfloat_p Wr, LWr;  // [C][reps*S*S]
    float *out;
    double *ll_sum;
    int ll_cnt;        // index of the count behind ll_sum: 1, or 16 with DPK_FLAG_LL_SUM_SPREAD
    // exact evaluation
    const int64_t *mask;
    const uint8_t *pad;
    const float *loc, *scale;
#ifdef DPK_TIMELINE
    unsigned long long *dbg;   // [blocks][waves][64][8] s_memtime stamps (measurement builds)
#endif
    int ablate;       // measurement only (DPK_GEMM_ABLATE): 1 no compute, 2 no table DMA, 4 no x DMA
    int *slow_flag;   // host-mapped hint word (may be null): launch number of the last launch that met NaN evidence
    int launch_seq;
};

__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2) {
    const float mm = fmaxf(m, m2);
    if (mm == -INFINITY) {
        s = 0.f;
        return;
    }
    s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
    m = mm;
}


// ---- exp-domain helpers of the fast upper layers ---------------------------------------------------------------
// e[i] = 2^((x[i] - max) log2 e); returns max (0 for an all -inf input, whose exponentials are then 0)
template <int NI> __device__ __forceinline__ float exp2_children(const float (&x)[NI], float (&e)[NI]) {
    float m = x[0];
#pragma unroll
    for (int i = 1; i < NI; ++i) m = fmaxf(m, x[i]);
    const float m0 = (m == -INFINITY) ? 0.f : m;
#pragma unroll
    for (int i = 0; i < NI; ++i) e[i] = __builtin_amdgcn_exp2f((x[i] - m0) * 1.4426950408889634f);
    return m0;
}

// Exact per-element evaluation of the 32 samples of a wave (any scale, any evidence): lane (s, h) takes the
// repetitions rho = 2m + h, the two lanes of a sample meet in one shuffle per class.  Slow by design.
template <int I, int S, int NT>
__device__ __noinline__ void gemm_exact_wave(const GemmArgs &a, int64_t bw0, int lane, LseScratch sc) {
    constexpr int RPT = 8 / I;
    constexpr int RH = (NT * RPT + 1) / 2;   // repetitions per lane half
    const int s = lane & 31, h = lane >> 5;
    const int64_t b = bw0 + s;
    const bool valid = b < a.B;
    const float *xr = a.x + (valid ? b : a.B - 1) * a.D;
    const int d = a.d;
    float n1[RH][2][S];
#pragma unroll
    for (int m = 0; m < RH; ++m) {
        const int rho = 2 * m + h;
        float leaf[4][I];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < I; ++k) leaf[q][k] = 0.f;
        if (rho < a.reps) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = rho * 4 + q;
                for (int j = 0; j < d; ++j) {
                    const int64_t o = (int64_t)r * d + j;
                    if (a.pad != nullptr && a.pad[o]) continue;
                    const float xv = xr[a.mask[o]];
#pragma unroll
                    for (int k = 0; k < I; ++k) {
                        const int64_t po = ((int64_t)r * I + k) * d + j;
                        const float mu = a.loc[po], sg = a.scale[po];
                        const float dlt = xv - mu;
                        leaf[q][k] += nan_to_num_f(fmaf(dlt * dlt, -0.5f / (sg * sg), -logf(sg) - kLogSqrt2Pi));
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int64_t wo = ((int64_t)rho * 2 + p) * S * I * I;
                prodsum_node<I, S>(leaf[2 * p], leaf[2 * p + 1], a.W0 + wo, a.LW0 + wo, sc, n1[m][p]);
            }
        }
    }
    const int M = a.reps * S * S;
    double part = 0.0;
    for (int cl = 0; cl < a.C; ++cl) {
        float mm = -INFINITY, ss = 0.f;
#pragma unroll
        for (int m = 0; m < RH; ++m) {
            const int rho = 2 * m + h;
            if (rho < a.reps) {
                float ea[S], ec[S], ma, mc, pm, ps;
                exp_children<S>(n1[m][0], ea, ma);
                exp_children<S>(n1[m][1], ec, mc);
                const float *wr = (const float *)a.Wr + (int64_t)cl * M + rho * S * S;
                const float *lwr = (const float *)a.LWr + (int64_t)cl * M + rho * S * S;
                root_partial<S>(n1[m][0], n1[m][1], ea, ec, ma, mc, wr, lwr, sc, pm, ps);
                lse_merge(mm, ss, pm, ps);
            }
        }
        const float om = __shfl_xor(mm, 32, 64), os = __shfl_xor(ss, 32, 64);
        lse_merge(mm, ss, om, os);
        const float ll = (mm > -INFINITY) ? mm + logf(ss) : -INFINITY;
        if (h == 0 && valid) {
            a.out[b * a.C + cl] = ll;
            part += (double)ll;
        }
    }
    if (a.ll_sum != nullptr) {
        part = wave_reduce_sum(part);
        if (lane == 0) atomicAdd(a.ll_sum, part);   // (the count: once per launch, at the end of the kernel)
    }
}

// The table-free evaluation of a launch that found its tables stale: gemm_exact_wave with the log-softmax weights taken
// straight from the raw sum / root weights (the tables are being rebuilt).
template <int I, int S, int NT>
__device__ __noinline__ void gemm_exact_wave_raw(const GemmArgs &a, const float *raw0, const float *rawr, int64_t bw0, int lane,
                                                 LseScratch sc) {
    constexpr int RPT = 8 / I;
    constexpr int RH = (NT * RPT + 1) / 2;
    const int s = lane & 31, h = lane >> 5;
    const int64_t b = bw0 + s;
    const bool valid = b < a.B;
    const float *xr = a.x + (valid ? b : a.B - 1) * a.D;
    const int d = a.d;
    float n1[RH][2][S];
#pragma unroll
    for (int m = 0; m < RH; ++m) {
        const int rho = 2 * m + h;
        float leaf[4][I];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < I; ++k) leaf[q][k] = 0.f;
        if (rho < a.reps) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = rho * 4 + q;
                for (int j = 0; j < d; ++j) {
                    const int64_t o = (int64_t)r * d + j;
                    if (a.pad != nullptr && a.pad[o]) continue;
                    const float xv = xr[a.mask[o]];
#pragma unroll
                    for (int k = 0; k < I; ++k) {
                        const int64_t po = ((int64_t)r * I + k) * d + j;
                        const float mu = a.loc[po], sg = a.scale[po];
                        const float dlt = xv - mu;
                        leaf[q][k] += nan_to_num_f(fmaf(dlt * dlt, -0.5f / (sg * sg), -logf(sg) - kLogSqrt2Pi));
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 2; ++p)
                prodsum_node_raw<I, S>(leaf[2 * p], leaf[2 * p + 1], raw0 + ((int64_t)rho * 2 + p) * S * I * I, sc.slot, n1[m][p]);
        }
    }
    const int M = a.reps * S * S;
    double part = 0.0;
    for (int cl = 0; cl < a.C; ++cl) {
        const float lse_row = raw_row_lse(rawr + (int64_t)cl * M, M);
        float mm = -INFINITY, ss = 0.f;
#pragma unroll
        for (int m = 0; m < RH; ++m) {
            const int rho = 2 * m + h;
            if (rho < a.reps) {
                float pm, ps;
                root_partial_raw<S>(n1[m][0], n1[m][1], rawr + (int64_t)cl * M + rho * S * S, lse_row, sc.slot, pm, ps);
                lse_merge(mm, ss, pm, ps);
            }
        }
        const float om = __shfl_xor(mm, 32, 64), os = __shfl_xor(ss, 32, 64);
        lse_merge(mm, ss, om, os);
        const float ll = (mm > -INFINITY) ? mm + logf(ss) : -INFINITY;
        if (h == 0 && valid) {
            a.out[b * a.C + cl] = ll;
            part += (double)ll;
        }
    }
    if (a.ll_sum != nullptr) {
        part = wave_reduce_sum(part);
        if (lane == 0) atomicAdd(a.ll_sum, part);
    }
}

#ifdef DPK_TIMELINE
#define GEMM_STAMP(row, slot) do { __builtin_amdgcn_sched_barrier(0); if (a.dbg && lane == 0 && !loader && (row) < 64) a.dbg[(((int64_t)blockIdx.x * kGemmWaves + wave) * 64 + (row)) * 8 + (slot)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define GEMM_STAMP(row, slot) do { } while (0)
#endif

#define RING_VI 0
#define RING_KERNEL_NAME ratspn_gemm_kernel
#define RING_KERNEL_PARAMS const GemmArgs a
#include "ratspn_gemm_ring_kernel.inc"
#undef RING_VI
#undef RING_KERNEL_NAME
#undef RING_KERNEL_PARAMS
#define RING_VI 1
#define RING_KERNEL_NAME ratspn_gemm_vi_kernel
#define RING_KERNEL_PARAMS const GemmArgs a, const GemmPrepArgs pv
#include "ratspn_gemm_ring_kernel.inc"
#undef RING_VI
#undef RING_KERNEL_NAME
#undef RING_KERNEL_PARAMS

}  // namespace ring

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
template <int I, int S, int NT>
static int gemm_launch(const ring::GemmArgs &a, int reps, hipStream_t st, const GemmPrepArgs *vi = nullptr) {
    constexpr int KS = gemm_ks(NT);
    constexpr int BB = KS * NT * 2 * 1024;
    constexpr int NMAX = (I > S ? I : S);
    const size_t lds = (size_t)kGemmStages * (kGemmTile * 64 * KS + BB) +
                       (size_t)(2 * NT * 16 + reps * 2 * S * I * I) * 4 + (size_t)kGemmWaves * 64 * 2 * NMAX * 4 + (vi ? 64 : 0);
    DPK_REQUIRE(lds <= 160 * 1024, DPK_EUNSUPPORTED, "ratspn_gemm: %zu bytes of LDS", lds);
    const int cus = device_cus();
    const int grid = a.ntiles < cus ? a.ntiles : cus;
    if (vi != nullptr) {
        // the launch checks its parameter tables itself (ratspn_gemm_prep.h): table work on the compute waves of the
        // first np work-groups, one verdict reader per work-group
        auto kvi = ring::ratspn_gemm_vi_kernel<I, S, NT>;
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kvi), 160 * 1024 - 256)) return rc;
        GemmPrepArgs pv = *vi;
        pv.readers = grid;
        {   // (measurement: DPK_RING_VI_NP0=1 runs the self-checking kernel without its table work)
            static const bool np0 = [] { const char *e = getenv("DPK_RING_VI_NP0"); return e && atoi(e) != 0; }();
            if (np0) pv.np = 0;
        }
        Profile prof(DPK_KERNEL_RATSPN_FUSED, st);
        DPK_LAUNCH_IN(prof, "ratspn_gemm_kernel (self-checking)", kvi, dim3(grid), dim3(2 * kGemmWaves * 64), lds, st,
                      a, pv);
        return DPK_OK;
    }
    auto kern = ring::ratspn_gemm_kernel<I, S, NT>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), 160 * 1024)) return rc;
#ifdef DPK_TIMELINE
    const_cast<ring::GemmArgs &>(a).dbg = timeline_buffer("", (size_t)1024 * kGemmWaves * 64 * 8 * 8, grid, a.NCH);
#endif
    Profile prof(DPK_KERNEL_RATSPN_FUSED, st);
    DPK_LAUNCH_IN(prof, "ratspn_gemm_kernel", kern, dim3(grid), dim3(2 * kGemmWaves * 64), lds, st, a);
    return DPK_OK;
}

template <int I, int S>
static int gemm_dispatch_nt(const ring::GemmArgs &a, int reps, int NT, hipStream_t st, const GemmPrepArgs *vi) {
    switch (NT) {
        case 1: return gemm_launch<I, S, 1>(a, reps, st, vi);
        case 2: return gemm_launch<I, S, 2>(a, reps, st, vi);
        case 3: return gemm_launch<I, S, 3>(a, reps, st, vi);
        case 4: return gemm_launch<I, S, 4>(a, reps, st, vi);
    }
    set_error("ratspn_gemm: %d column tiles not built", NT);
    return DPK_EUNSUPPORTED;
}

// ratspn_gemm_small.hip: 32-sample tiles, features split over the waves (small batches);
// ratspn_gemm_nan.hip: the ring kernel's variant for marginalised evidence
bool gemm_small_shape_ok(int D, int NT);
int64_t gemm_small_max_batch();
int ratspn_gemm_small_forward(const GemmArgs &a, const GemmPrepArgs &p, int reps, int I, int S, int NT, hipStream_t st);
bool gemm_marginal_shape_ok(int D, int NT);
// ratspn_gemm_slice.hip: persistent 32-sample blocks, the feature axis split over seven waves with the mean table in registers
bool gemm_slice_shape_ok(int D, int reps, int I, int S, int NT);
int64_t gemm_slice_min_batch();
int ratspn_gemm_slice_forward(const GemmArgs &a, const GemmPrepArgs &p, int I, int S, int NT, int lanes, hipStream_t st);
int gemm_slice_lanes(const void *ws_key, uint32_t flags, hipStream_t st);   // this launch and the launches beside it
bool gemm_slice_checks_inline(int64_t B, int np, int d, int lanes);
// ratspn_gemm_wide.hip: 8-channel models, a wave per repetition
bool gemm_wide_shape_ok(int D, int reps, int I, int S, int C);
int ratspn_gemm_wide_forward(const GemmArgs &a, const GemmPrepArgs &p, int S, hipStream_t st);
bool gemm_wide_takes_tile32(int64_t B, int D, int reps, int C, bool marginal, bool emit);
int ratspn_gemm_marginal_forward(const GemmArgs &a, int reps, int I, int S, int NT, hipStream_t st);

// The caller (dpk_ratspn_forward) has validated the arguments and carved the workspace.
int ratspn_gemm_forward(const RatWs &w, const float *x, int64_t B, int D, const int64_t *mask, const uint8_t *pad,
                        const float *loc, const float *scale, const float *sum_weight0, const float *root_weight,
                        int reps, int I, int S, int C, float *out, double *ll_sum, uint32_t flags, hipStream_t st,
                        const GemmEmit *emit) {
    const int d = (D + (4 - D % 4) % 4) / 4;
    const int NT = w.g_nt;
    int *slow_word = nullptr;
    int launch_seq = 0;
    bool marginal = slow_hint_next(w.gm_tab, &slow_word, &launch_seq);   // (keyed by this workspace's tables)
    static const int ablate = [] { const char *e = getenv("DPK_GEMM_ABLATE"); return e ? atoi(e) : 0; }();
    {   // (measurement: DPK_GEMM_MARGINAL=0 / 1 pins the variant)
        static const int force = [] { const char *e = getenv("DPK_GEMM_MARGINAL"); return e ? atoi(e) : -1; }();
        if (force >= 0) marginal = force != 0;
    }
    // Three mappings of the same arithmetic: below ~one 128-sample tile per compute unit the persistent ring kernel
    // runs at the latency of its chunk walk and 32-sample tiles with the feature axis split over the waves take over
    // (ratspn_gemm_small.hip); while recent launches met NaN evidence the ring variant that stages both tables runs
    // (ratspn_gemm_nan.hip); otherwise the ring kernel below.
    const bool wide = I == 8;
    const bool emitting = emit != nullptr;
    const bool marginal_ring = marginal && gemm_marginal_shape_ok(D, NT);
    // (the slice mapping: clean evidence only -- a block that meets NaN is evaluated exactly and sets the hint)
    const bool slice = !wide && !emitting && !marginal_ring && gemm_slice_min_batch() >= 0 && B >= gemm_slice_min_batch() &&
                       gemm_slice_shape_ok(D, reps, I, S, NT);
    // (how many launches share the compute units -- the caller's word, or what the other streams are doing: ratspn_gemm_slice.hip)
    const int slice_lanes = slice ? gemm_slice_lanes(w.gctl, flags, st) : 1;
    const bool small = !wide && !slice && B <= gemm_small_max_batch() && gemm_small_shape_ok(D, NT);
    if (emitting && !wide && !small) {   // (training forward: the 32-sample kernels)
        set_error("ratspn_forward_train: channels=%d at %lld samples not built (dpk_ratspn_small_batch_max)", I, (long long)B);
        return DPK_EUNSUPPORTED;
    }
    // The tables.  "Believed current -- check" (DPK_FLAG_PARAMS_VERIFY) costs the 32-sample mappings nothing extra: their
    // launch carries the table work-groups itself (kPrepInline, ratspn_gemm_prep.h).  The ring kernels keep the
    // stand-alone check launch in front of them (DPK_VERIFY_INLINE=0 forces it everywhere: A/B measurements).
    static const bool inline_allowed = [] { const char *e = getenv("DPK_VERIFY_INLINE"); return !(e && atoi(e) == 0); }();
    GemmPrepArgs p{};
    p.mask = mask; p.pad = pad; p.loc = loc; p.scale = scale;
    p.D = D; p.d = d; p.reps = reps; p.NT = NT; p.NKSP = w.g_nksp; p.KS = gemm_ks(NT);
    p.mtab = w.gm_tab; p.ctab = w.gc_tab; p.bias = w.gbias; p.bias_row = w.gbias_row; p.bias_ks = w.gbias_ks;
    p.bias_sl = w.gbias_sl; p.elig = w.gelig;
    p.w[0] = sum_weight0; p.W[0] = w.w[0]; p.LW[0] = w.lw[0]; p.rows[0] = reps * 2 * S; p.n[0] = I * I;
    p.w[1] = root_weight; p.W[1] = w.w[2]; p.LW[1] = w.lw[2]; p.rows[1] = C; p.n[1] = reps * S * S;
    p.hash = w.ghash; p.ctl = w.gctl;
    p.stab = w.gs_tab; p.smask = w.gs_mask;
    p.wx_part = w.gwx_part; p.wx_tick = w.gwx_tick;
    { static const int pab = [] { const char *e = getenv("DPK_PREP_ABLATE"); return e ? atoi(e) : 0; }(); p.ablate = pab; }
    p.upfrag = (I == 8 && S >= 2) ? w.gup : nullptr; p.up_S = S;
    const int np = gemm_prep_blocks(NT, I, p.rows[0] + p.rows[1], kGemmPrepThreads);
    const size_t prep_lds = gemm_prep_lds_bytes(D, I, d);
    DPK_REQUIRE(prep_lds <= 60 * 1024, DPK_EUNSUPPORTED, "ratspn_gemm: in_features=%d too large for the table kernel", D);
    // (the ring kernel: its table work rides on the compute waves of its first np work-groups -- it needs that many)
    const bool ring_plain = !wide && !small && !slice && !marginal_ring;
    // Measured (round 4, B = 65536, default-mode step): frozen kernel 47.4 us; kernel + stand-alone check launch 52.8 us;
    // self-checking ring kernel 58.8 us, 55.6 us even WITHOUT its table work (DPK_RING_VI_NP0=1) -- the verdict logic at
    // the first tile's upper layers is enough to cost the hot loop its register allocation (237 VGPRs, 71 spilled SGPRs
    // against 234 / 57).  So the ring kernel keeps the stand-alone launch; DPK_RING_VI=1 selects the variant (tests, A/B).
    static const bool ring_vi = [] { const char *e = getenv("DPK_RING_VI"); return e && atoi(e) != 0; }();
    const bool ring_inline = ring_vi && ring_plain && (int64_t)np <= std::min<int64_t>(cdiv(B, kGemmTile), device_cus());
    const bool verify_inline = inline_allowed && (flags & DPK_FLAG_PARAMS_VERIFY) && !(flags & DPK_FLAG_PARAMS_CACHED) &&
                               ((wide && gemm_wide_takes_tile32(B, D, reps, C, marginal, emitting)) || small || ring_inline ||
                                (slice && gemm_slice_checks_inline(B, np, p.d, slice_lanes)));
    if (verify_inline) {
        p.mode = kPrepInline;
        p.np = np;
    } else if (!(flags & DPK_FLAG_PARAMS_CACHED)) {
        p.mode = (flags & DPK_FLAG_PARAMS_VERIFY) ? kPrepVerify : kPrepBuild;
        if (I == 2) DPK_LAUNCH("ratspn_gemm_prep_kernel", ratspn_gemm_prep_kernel<2>, dim3(np), dim3(kGemmPrepThreads),
            prep_lds, st, p);
        else if (I == 4) DPK_LAUNCH("ratspn_gemm_prep_kernel", ratspn_gemm_prep_kernel<4>, dim3(np),
            dim3(kGemmPrepThreads), prep_lds, st, p);
        else DPK_LAUNCH("ratspn_gemm_prep_kernel", ratspn_gemm_prep_kernel<8>, dim3(np), dim3(kGemmPrepThreads),
            prep_lds, st, p);
        p.np = 0;
    }
    if (wide || small || slice || marginal_ring) {
        GemmArgs a{};
        a.x = x; a.B = B; a.D = D; a.d = d; a.reps = reps; a.C = C;
        a.NCH = cdiv(D, 16 * gemm_ks(NT));
        a.ntiles = cdiv(B, kGemmTile);
        a.mtab = w.gm_tab; a.ctab = w.gc_tab; a.biasT = w.gbias_row; a.biasC = w.gbias; a.elig = w.gelig;
        a.biasK = w.gbias_ks; a.biasS = w.gbias_sl;
        a.W0 = w.w[0]; a.LW0 = w.lw[0]; a.Wr = as_const(w.w[2]); a.LWr = as_const(w.lw[2]);
        a.out = out; a.ll_sum = ll_sum; a.ll_cnt = (flags & DPK_FLAG_LL_SUM_SPREAD) ? 16 : 1;
        a.mask = mask; a.pad = pad; a.loc = loc; a.scale = scale;
        a.slow_flag = slow_word; a.launch_seq = launch_seq; a.marginal = marginal ? 1 : 0;
        a.ablate = ablate;
        a.upfrag = p.upfrag;
        if (emitting) { a.emit_leaf = emit->leaf; a.emit_sum = emit->sum; a.emit_out = emit->out; }
        if (wide) return ratspn_gemm_wide_forward(a, p, S, st);
        if (small) return ratspn_gemm_small_forward(a, p, reps, I, S, NT, st);
        if (slice) return ratspn_gemm_slice_forward(a, p, I, S, NT, slice_lanes, st);
        return ratspn_gemm_marginal_forward(a, reps, I, S, NT, st);
    }
    ring::GemmArgs a{};
    a.x = x; a.B = B; a.D = D; a.d = d; a.reps = reps; a.C = C;
    a.NCH = cdiv(D, 16 * gemm_ks(NT));
    a.ntiles = cdiv(B, kGemmTile);
    a.mtab = w.gm_tab; a.ctab = w.gc_tab; a.biasT = w.gbias_row; a.biasC = w.gbias; a.elig = w.gelig;
    a.W0 = w.w[0]; a.LW0 = w.lw[0]; a.Wr = as_const(w.w[2]); a.LWr = as_const(w.lw[2]);
    a.out = out; a.ll_sum = ll_sum; a.ll_cnt = (flags & DPK_FLAG_LL_SUM_SPREAD) ? 16 : 1;
    a.mask = mask; a.pad = pad; a.loc = loc; a.scale = scale;
    a.slow_flag = slow_word; a.launch_seq = launch_seq;
    a.ablate = ablate;
    const GemmPrepArgs *vi = (verify_inline && ring_inline) ? &p : nullptr;
    if (I == 2) {
        if (S == 2) return gemm_dispatch_nt<2, 2>(a, reps, NT, st, vi);
        return gemm_dispatch_nt<2, 4>(a, reps, NT, st, vi);
    }
    if (S == 2) return gemm_dispatch_nt<4, 2>(a, reps, NT, st, vi);
    return gemm_dispatch_nt<4, 4>(a, reps, NT, st, vi);
}

}  // namespace dpk
