// RAT-SPN fused forward for 8-CHANNEL models (depth 2, unit-scale Gaussian leaves, rg_batch = 8, <= 8 repetitions):
// leaf layer on the matrix cores, product / sum / root layers in registers, one launch for any batch size.
//
// reference: RatSpn.forward (deeprob/spn/models/ratspn.py:105-122) = RegionGraphLayer.forward + GaussianLayer
// (deeprob/spn/layers/ratspn.py:87-108, :160-213), ProductLayer :272-286, SumLayer :363-378, RootLayer :446-458 at the
// sizes of experiments/ratspn.py (rg_batch = rg_sum = 8) -- BASELINE config 2's second line.
//
// Same formulation, tables and arithmetic as ratspn_gemm.hip (read its header first).  With 8 channels a repetition
// fills one 32-column MFMA tile (4 regions x 8 channels), so the mapping is by REPETITION instead of by feature slice:
//   * a work-group owns 32 samples (one MFMA column block); wave w owns repetition w: the whole K range of its column
//     tile, 16 accumulator registers, no partial sums to exchange.  The MFMA leaves lane (sample s, half h) with the 8
//     channels of regions {2h, 2h+1} of repetition w: exactly one partition's inputs, so the product + sum node of that
//     partition runs in the lane's registers, the partner partition arrives by one v_permlane32_swap per value and the
//     repetition's share of the root follows; only the root's log-sum-exp over the repetitions crosses waves (LDS);
//   * the x tile (100 KB at D = 784) is staged once in LDS by DMA ([K-step][row][64 bytes], source-side XOR swizzle as
//     in ratspn_gemm_small.hip), shared by the eight waves; each wave streams ITS tile's table fragments from L2 into
//     registers, a dozen K-steps ahead (the accumulators being 16 registers, the file is free for that);
//   * three kernels (leaf | product+sum | product+root), two [B, 32, 8] tensors between them and three table builds
//     become one launch and one table check.
// Marginalised evidence: while the NaN hint is up (slow_hint) the negated-constant fragments travel with the mean
// fragments; otherwise a K-step that holds NaN fetches them on demand.  +-inf / huge evidence, large sums of squares
// and models outside the expanded square's envelope: the wave evaluates its repetition's leaf sums exactly, per element
// (every wave sees the same x tile, so all eight take that decision together).  Vanished sum nodes fall back to the
// log domain inside prodsum_node / root_partial (ratspn_nodes.h).
#include "ratspn_gemm_fused.h"
#include "ratspn_gemm_prep.h"
#include <type_traits>
#include <stdlib.h>

namespace dpk {

constexpr int kWideWaves = 8;      // waves per work-group = repetitions (column tiles) it can hold
constexpr int kWideI = 8;
constexpr int kWideMaxC = 32;      // classes: the repetitions' root partials are exchanged through LDS

// The upper part of ONE 32-sample block on the eight compute waves of a work-group (wave = repetition): leaf sums of the
// lane's partition from its accumulators (or exactly, per element), the partition's product + sum node, the
// repetition's share of the root, the log-sum-exp over the repetitions through LDS and the store.  `lds` = scratch the
// block may overwrite (>= wide_upper_lds_bytes: per-lane log-domain scratch + the root exchange buffer).  Executes
// kWideUpperBarriers work-group barriers (waves without this work call wide_upper_barriers() instead).  Returns the
// thread's fp64 share of the sum of the log-likelihoods it stored.
constexpr int kWideUpperBarriers = 2;
__device__ __forceinline__ void wide_upper_barriers() {
#pragma unroll
    for (int i = 0; i < kWideUpperBarriers; ++i) __syncthreads();
}
__host__ __device__ constexpr size_t wide_upper_lds_bytes(int reps, int C) {
    return (size_t)kWideWaves * 64 * 2 * kWideI * 4 + ((size_t)reps * 32 * C * 2 + 32) * 4;
}

// Leaf sums of the lane's partition -- regions 2h (va) and 2h + 1 (vc) of repetition rho, for sample b0 + s -- from the
// block's accumulators, or exactly, per element (any scale, any evidence).
__device__ __forceinline__ void wide_leaf_sums(const GemmArgs &a, const gf32x16 &acc, unsigned long long odd_mask, bool exact,
                                               int rho, int64_t b0, float (&va)[kWideI], float (&vc)[kWideI]) {
    constexpr int I = kWideI;
    const int lane = threadIdx.x & 63;
    const int s = lane & 31, h = lane >> 5;
    const int D = a.D, NT = a.reps, NKS = (D + 15) >> 4;
    const int64_t b = b0 + s;
    if (!exact) {
        float cst[16];
        if (odd_mask == 0ull) {
            const float *bt = a.biasT + (h * NT + rho) * 16;
#pragma unroll
            for (int i = 0; i < 16; ++i) cst[i] = bt[i];
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) cst[i] = 0.f;
            for (int ks = 0; ks < NKS; ++ks) {
                if ((odd_mask >> ks) & 1ull) continue;
                const float *bk = a.biasK + ((ks * 2 + h) * NT + rho) * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) cst[i] += bk[i];
            }
        }
#pragma unroll
        for (int k = 0; k < I; ++k) {
            va[k] = acc[k] + cst[k];                       // (the common -1/2 sum x^2 reaches the root as qtot)
            vc[k] = acc[I + k] + cst[I + k];
        }
    } else {
        // exact per-element evaluation of the partition's two regions (nan_to_num_ at ratspn.py:103)
        const float *xr = a.x + (b < a.B ? b : a.B - 1) * D;
        const int d = a.d;
#pragma unroll
        for (int k = 0; k < I; ++k) {
            va[k] = 0.f;
            vc[k] = 0.f;
        }
        for (int qq = 0; qq < 2; ++qq) {
            const int r = rho * 4 + 2 * h + qq;
            float t[I];
#pragma unroll
            for (int k = 0; k < I; ++k) t[k] = 0.f;
            for (int j = 0; j < d; ++j) {
                const int64_t o = (int64_t)r * d + j;
                if (a.pad != nullptr && a.pad[o]) continue;
                const float xv = xr[a.mask[o]];
#pragma unroll
                for (int k = 0; k < I; ++k) {
                    const int64_t po = ((int64_t)r * I + k) * d + j;
                    const float mu = a.loc[po], sg = a.scale[po];
                    const float dlt = xv - mu;
                    t[k] += nan_to_num_f(fmaf(dlt * dlt, -0.5f / (sg * sg), -logf(sg) - kLogSqrt2Pi));
                }
            }
#pragma unroll
            for (int k = 0; k < I; ++k) {
                if (qq == 0) va[k] = t[k]; else vc[k] = t[k];
            }
        }
    }
}

// The wave's MFMA fragments of its repetition's first sum layer (ratspn_gemm_prep.h wide_upfrag_*), requested by the
// caller ahead of the upper part (an L2 round trip inside it would sit on the critical path of every block).
template <int S> struct WideUpFrags {
    static constexpr int TILES = S / 2 > 0 ? S / 2 : 1;
    half8 hi[TILES], lo[TILES];
    __device__ __forceinline__ void load(const GemmArgs &a, int rho, int lane) {
        typedef const __attribute__((address_space(1))) half8 gh8u;
        if (a.upfrag == nullptr) return;
        const gh8u *fp = (const gh8u *)(a.upfrag + (int64_t)rho * TILES * 1024) + lane;
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            hi[t] = fp[t * 128];
            lo[t] = fp[t * 128 + 64];
        }
    }
};

// raw0 / rawr non-null: a launch that found its tables stale (ratspn_gemm_prep.h; `exact` is then set as well) -- the
// nodes take their log-softmax weights straight from the raw sum / root weights.
// NW = 4: the block is shared by TWO work-groups of four waves, repetitions [4 g, 4 g + 4) each (the 32-sample kernel at
// batches that would otherwise leave half the chip idle).  Each leaves its (max, sum) root partials in its slot of the
// workspace (xpart), performed before it draws the block's ticket (xtick: two draws per launch and block, then reset by the
// second arriver); the work-group that draws the odd ticket merges the other's partials with its own and stores.
template <int S, bool PRE = true, bool EMIT = false, int NW = kWideWaves>
__device__ __forceinline__ double wide_block_upper(const GemmArgs &a, const gf32x16 &acc, unsigned long long odd_mask,
                                                   float qtot, bool exact, int rho, bool mine, int64_t b0,
                                                   const lfloat *w0_l, char *lds, const WideUpFrags<S> &uf,
                                                   const float *raw0 = nullptr, const float *rawr = nullptr,
                                                   float *xpart = nullptr, unsigned *xtick = nullptr, int grp = 0) {
    constexpr int I = kWideI;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = lane & 31, h = lane >> 5;
    const int NT = a.reps;
    if constexpr (NW < kWideWaves) {
        if (wave >= NW) {   // (the x-tile helpers of a shared block: the four barriers of the path below)
#pragma unroll
            for (int i = 0; i < ((a.ablate & 2) ? kWideUpperBarriers : 4); ++i) __syncthreads();
            return 0.0;
        }
    }
    // ---- leaf sums of the lane's partition: regions 2h (a) and 2h + 1 (c) of repetition rho -------------------------
    float va[I], vc[I];
    wide_leaf_sums(a, acc, odd_mask, exact, rho, b0, va, vc);
    if constexpr (EMIT) {
        // (training forward: the lane's two regions are 16 consecutive floats of the [B, R, I] leaf tensor)
        if (mine && b0 + s < a.B) {
            gf32x4 *dst = reinterpret_cast<gf32x4 *>(a.emit_leaf + ((b0 + s) * (4 * NT) + rho * 4 + 2 * h) * I);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const gf32x4 v0 = {va[4 * q], va[4 * q + 1], va[4 * q + 2], va[4 * q + 3]};
                const gf32x4 v1 = {vc[4 * q], vc[4 * q + 1], vc[4 * q + 2], vc[4 * q + 3]};
                dst[q] = v0;
                dst[2 + q] = v1;
            }
        }
    }
    if (a.ablate & 2) {
        wide_upper_barriers();
        return 0.0;
    }

    // ---- the partition's product + sum node, then the repetition's share of the root ---------------------------------
    LseScratch sc{reinterpret_cast<float *>(lds) + tid * (2 * I)};                  // [512][16] floats = 32 KB
    float *xch = reinterpret_cast<float *>(lds) + kWideWaves * 64 * 2 * I;           // [reps][32][2 C]
    float n1[S];
    {
        const lfloat *wl = w0_l + h * S * I * I;
        const float *lw = a.LW0 + ((int64_t)rho * 2 + h) * S * I * I;
        if (raw0 != nullptr) {
            prodsum_node_raw<I, S>(va, vc, raw0 + ((int64_t)rho * 2 + h) * S * I * I, sc.slot, n1);
        } else if (PRE && a.upfrag != nullptr && !(a.ablate & 32)) {
            // Round 4: the repetition's two product + sum nodes as ONE small GEMM on the matrix cores (fragment layout:
            // ratspn_gemm_prep.h wide_upfrag_*): T[(h, o, i), s] = sum_j W[h][o][i][j] e^{c_j - max c}, the partition h in
            // the K index -- lane half h of the B operand holds its own partition's exponentials as they fall out of the
            // leaf GEMM -- then the lane's dot product with e^{a_i - max a}: 3 S/2 MFMAs + 8 S FMAs per lane instead of
            // 72 S FMAs and 16 S broadcast LDS reads.  Operands in [0, 1] scaled by 2^15 before the f16 split, 2^-30
            // after (ratspn_upper_gemm.hip); a node below 1e-8 sends the wave through the log-domain-safe form.
            constexpr int TILES = WideUpFrags<S>::TILES;
            constexpr float kL2E = 1.4426950408889634f, kLn2 = 0.6931471805599453f;
            // (PRE: the 32-sample kernel, whose caller requested the fragments ahead of the upper part.  The ring kernel
            // keeps the vector-ALU form below: with four blocks' accumulators live, the GEMM form's operands spilled 80-130
            // registers to scratch at its 168-register budget and measured 7 us per tile SLOWER -- round 4, not kept.)
            float ma = va[0], mc = vc[0];
#pragma unroll
            for (int k = 1; k < I; ++k) {
                ma = fmaxf(ma, va[k]);
                mc = fmaxf(mc, vc[k]);
            }
            ma = (ma == -INFINITY) ? 0.f : ma;
            mc = (mc == -INFINITY) ? 0.f : mc;
            float ea[I], eb[I];
#pragma unroll
            for (int k = 0; k < I; ++k) {
                ea[k] = __builtin_amdgcn_exp2f((va[k] - ma) * kL2E);
                eb[k] = __builtin_amdgcn_exp2f(fmaf(vc[k] - mc, kL2E, 15.f));      // e^{c - max c} * 2^15
            }
            half8 eh, el8;
            split8(eb, eh, el8);
            bool vanished = false;
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                gf32x16 tt;
#pragma unroll
                for (int i = 0; i < 16; ++i) tt[i] = 0.f;
                const half8 fh = uf.hi[t], fl = uf.lo[t];
                tt = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh, eh, tt, 0, 0, 0);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_f16(fh, el8, tt, 0, 0, 0);
                tt = __builtin_amdgcn_mfma_f32_32x32x16_f16(fl, eh, tt, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (2 * t + q < S) {
                        float v = 0.f;
#pragma unroll
                        for (int i = 0; i < I; ++i) v = fmaf(ea[i], tt[q * 8 + i], v);
                        v *= 1.f / (kWideUpScale * kWideUpScale);
                        vanished = vanished || (v < 1e-8f);
                        n1[2 * t + q] = fmaf(__builtin_amdgcn_logf(v), kLn2, ma + mc);
                    }
                }
            }
            if (__any(vanished)) prodsum_node<I, S>(va, vc, wl, lw, sc, n1);   // (rare: vanishing weight on the dominant pair)
        } else {
            prodsum_node<I, S>(va, vc, wl, lw, sc, n1);
        }
    }
    if constexpr (EMIT) {
        if (mine && b0 + s < a.B) {
            float *dst = a.emit_sum + ((b0 + s) * (2 * NT) + rho * 2 + h) * S;
#pragma unroll
            for (int o = 0; o < S; ++o) dst[o] = n1[o];
        }
    }
    float ta[S], tc[S];
#pragma unroll
    for (int o = 0; o < S; ++o) {
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const unsigned bits = __float_as_uint(n1[o]);
        const u32x2 sw2 = __builtin_amdgcn_permlane32_swap(bits, bits, false, false);
        ta[o] = __uint_as_float(sw2[0]);
        tc[o] = __uint_as_float(sw2[1]);
    }
    float ea[S], ec[S], ma, mc;
    exp_children<S>(ta, ea, ma);
    exp_children<S>(tc, ec, mc);
    const int M = NT * S * S, C = a.C;
    if (mine) {
        // the two lanes of a sample hold the same (ta, tc): they split the classes
        for (int cl = h; cl < C; cl += 2) {
            float pm, ps;
            if (rawr != nullptr) {
                root_partial_raw<S>(ta, tc, rawr + (int64_t)cl * M + rho * S * S, raw_row_lse(rawr + (int64_t)cl * M, M),
                                    sc.slot, pm, ps);
            } else {
                const cfloat_p wr = a.Wr + (int64_t)cl * M + rho * S * S;
                const cfloat_p lwr = a.LWr + (int64_t)cl * M + rho * S * S;
                root_partial<S>(ta, tc, ea, ec, ma, mc, wr, lwr, sc, pm, ps);
            }
            if (!(ps > 0.f)) pm = -INFINITY;
            xch[((rho * 32 + s) * C + cl) * 2] = pm;
            xch[((rho * 32 + s) * C + cl) * 2 + 1] = ps;
        }
    }
    // sum x^2 of the sample: computed by the lanes (s, h = 0 / 1) of every wave; the root takes wave 0's through LDS
    float *qx = xch + NT * 32 * C * 2;
    if (wave == 0 && h == 0) qx[s] = exact ? 0.f : -0.5f * qtot;       // (the exact leaf sums already carry it)
    __syncthreads();                                   // (barrier 1 of kWideUpperBarriers)
    // ---- root: log-sum-exp over the repetitions; thread = (sample, class slot) ---------------------------------------
    double part = 0.0;
    if constexpr (NW == kWideWaves) {
        const int smp = tid >> 4, slot = tid & 15;
        const int64_t bs = b0 + smp;
        const float qterm = qx[smp];
        for (int cl = slot; cl < C; cl += 16) {
            float mm = -INFINITY, ss = 0.f;
            for (int r = 0; r < NT; ++r) lse_merge(mm, ss, xch[((r * 32 + smp) * C + cl) * 2], xch[((r * 32 + smp) * C + cl) * 2 + 1]);
            const float rel = (mm > -INFINITY) ? mm + logf(ss) : -INFINITY;
            const float ll = rel + qterm;
            if (bs < a.B) {
                a.out[bs * C + cl] = ll;
                if constexpr (EMIT) a.emit_out[bs * C + cl] = rel;
                part += (double)ll;
            }
        }
    } else {
        static_assert(NW == 4, "two work-groups per block");
        typedef unsigned long long u64;
        const int r0 = grp * NW, r1 = min(NT, r0 + NW);
        u64 *mine_x = reinterpret_cast<u64 *>(xpart) + (int64_t)grp * 32 * C;
        const u64 *other_x = reinterpret_cast<const u64 *>(xpart) + (int64_t)(1 - grp) * 32 * C;
        int *tick_l = reinterpret_cast<int *>(qx + 32);
        // this work-group's partials: kept in registers for the merge, and left where the other one finds them
        constexpr int kMaxPer = (32 * kWideMaxC + NW * 64 - 1) / (NW * 64);
        float pm[kMaxPer], ps[kMaxPer];
#pragma unroll
        for (int i = 0; i < kMaxPer; ++i) {
            const int e = i * NW * 64 + tid;
            pm[i] = -INFINITY;
            ps[i] = 0.f;
            if (e < 32 * C) {
                const int smp = e / C, cl = e - smp * C;
                for (int r = r0; r < r1; ++r)
                    lse_merge(pm[i], ps[i], xch[((r * 32 + smp) * C + cl) * 2], xch[((r * 32 + smp) * C + cl) * 2 + 1]);
                __hip_atomic_store(mine_x + e, ((u64)__float_as_uint(ps[i]) << 32) | __float_as_uint(pm[i]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the partials are PERFORMED before the ticket is drawn)
        __syncthreads();
        if (tid == 0) *tick_l = (int)__hip_atomic_fetch_add(xtick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if ((*tick_l & 1) != 0) {   // the second of the two: the other's partials are there
            // (both arrivals of this launch are in: the ticket goes back to zero, so that a launch that was aborted between
            // its two arrivals costs the NEXT launch this block once instead of shifting the parity for good -- ADVICE r05;
            // two streams on one workspace remain outside the contract: a workspace's launches follow one another)
            if (tid == 0) __hip_atomic_store(xtick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int i = 0; i < kMaxPer; ++i) {
                const int e = i * NW * 64 + tid;
                if (e < 32 * C) {
                    const int smp = e / C, cl = e - smp * C;
                    const u64 o = __hip_atomic_load(other_x + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    float mm = pm[i], ss = ps[i];
                    lse_merge(mm, ss, __uint_as_float((unsigned)o), __uint_as_float((unsigned)(o >> 32)));
                    const float rel = (mm > -INFINITY) ? mm + logf(ss) : -INFINITY;
                    const float ll = rel + qx[smp];
                    const int64_t bs = b0 + smp;
                    if (bs < a.B) {
                        a.out[bs * C + cl] = ll;
                        if constexpr (EMIT) a.emit_out[bs * C + cl] = rel;
                        part += (double)ll;
                    }
                }
            }
        }
    }
    __syncthreads();                                   // (barrier 2: the scratch may be overwritten by the next block)
    return part;
}

constexpr unsigned short kWideNanMark = 0x7E00;       // f16 quiet NaN: the low half of a value that is missing
struct WideTail {                                     // LDS behind the x tile and the weight slices: the waves' shares
    unsigned long long odd[kWideWaves];               // K-steps (of those the wave converted) that hold flagged values
    float qpart[kWideWaves][64];                      // sum x^2 of the lane's 8 features over those K-steps
    int flags[kWideWaves];                            // 1: out-of-range value (exact evaluation), 2: NaN seen
    int verdict;                                      // the launch found its parameter tables stale (ratspn_gemm_prep.h)
    int pad[3];
};
static_assert(sizeof(WideTail) % 16 == 0, "LDS layout");

// NW = 8: a work-group per block, wave = repetition.  NW = 4: two work-groups per block, repetitions [4 g, 4 g + 4) each on
// waves 0..3 -- at up to cus / 2 blocks (B <= 4096) the other form leaves half the chip idle with two repetitions' MFMA
// streams and upper layers per SIMD.  Still eight waves per work-group (the in-launch table work-groups are built for that;
// waves 4..7 help to stage and convert the x tile, then only keep the barriers); both work-groups stage the block's x
// tile (the second read is an Infinity-Cache hit) and meet at the root (wide_block_upper).
template <int S, bool MARG, bool EMIT, int NW>
__global__ __launch_bounds__(kWideWaves * 64) void ratspn_gemm_wide_kernel(const GemmArgs a, const GemmPrepArgs pa) {
    constexpr int I = kWideI;
    constexpr int PF = MARG ? 6 : 12;                 // K-steps of table fragments in flight per wave
    typedef const __attribute__((address_space(1))) half8 gh8;
    typedef __attribute__((address_space(3))) const gf32x4 lf4;
    typedef __attribute__((address_space(3))) half8 lh8;
    typedef __attribute__((address_space(3))) WideTail ltail;
    typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

    extern __shared__ __attribute__((aligned(16))) char smem_generic[];
    lchar *smem = (lchar *)smem_generic;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = lane & 31, h = lane >> 5;
    // A launch that checks its parameter tables itself (kPrepInline, ratspn_gemm_prep.h): the first pa.np work-groups are
    // the table work-groups -- fingerprint, verdict, rebuild if stale -- the others evaluate block blockIdx.x - pa.np.
    const int np = pa.np;
    if ((int)blockIdx.x < np) {
        gemm_prep_block_inline<kWideI>(pa, (int)blockIdx.x, reinterpret_cast<int *>(smem_generic));
        return;
    }
    const int D = a.D, NT = a.reps;
    const int NKS = (D + 15) >> 4;
    const int mb = (int)blockIdx.x - np;               // model work-group
    // (NW = 4: the two work-groups of a block stage the same x tile -- consecutive work-groups go to different XCDs, each
    // with its own L2, so the pair is work-groups L and L + 8: the second read of the tile is an L2 hit.  The host pads the
    // grid to whole groups of 16; work-groups beyond the last block leave at once.)
    const int grp = NW == kWideWaves ? 0 : ((mb >> 3) & 1);   // which half of the repetitions
    const int blk = NW == kWideWaves ? mb : ((mb >> 4) * 8 + (mb & 7));
    if (NW < kWideWaves && (int64_t)blk * 32 >= a.B) return;
    const int64_t b0 = (int64_t)blk * 32;
    const int nvalid = (int)min((int64_t)32, a.B - b0);
    const bool compute = wave < NW;                    // (NW = 4: waves 4..7 only help with the x tile)
    const bool mine = compute && grp * NW + wave < NT; // (a model with fewer repetitions leaves waves without a tile)
    const int rho = mine ? grp * NW + wave : NT - 1;
    // LDS: [0, NKS * 2048) the x tile; behind it the wave's copy of its two partitions' sum weights (2 x S x 64 floats)
    lfloat *w0_l = (lfloat *)(smem + NKS * 2048) + wave * (2 * S * I * I);

    // ---- requests: the x tile (every wave its share of the K-steps), then the first PF K-steps of fragments ----------
    {
        const gcchar_p xt = (gcchar_p)(a.x + b0 * D);
        unsigned voff[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int P = i * 64 + lane, row = P >> 2, c = (P & 3) ^ ((row >> 2) & 3);
            voff[i] = (unsigned)(min(row, nvalid - 1) * D + c * 4) * 4u;
        }
        for (int ks = wave; ks < NKS; ks += kWideWaves) {
            const int f0 = ks * 16;
            const unsigned dst = (unsigned)(uintptr_t)smem + ks * 2048;
            if (f0 + 16 <= D) {
                glds16(voff[0] + f0 * 4u, xt, dst);
                glds16(voff[1] + f0 * 4u, xt, dst + 1024);
            } else {   // ragged last K-step: pieces beyond the row re-fetch its first one (zeroed by the consumer)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int P = i * 64 + lane, row = P >> 2, c = (P & 3) ^ ((row >> 2) & 3);
                    const bool in = f0 + c * 4 + 4 <= D;
                    glds16(in ? voff[i] + f0 * 4u : (unsigned)(min(row, nvalid - 1) * D) * 4u, xt, dst + i * 1024);
                }
            }
        }
    }
    half8 mh[PF], ml[PF], ch[MARG ? PF : 1], cl[MARG ? PF : 1];
    const gcchar_p tbase = (gcchar_p)a.mtab + ((int64_t)rho * 2048 + lane * 16);
    const gcchar_p cbase = (gcchar_p)a.ctab + ((int64_t)rho * 2048 + lane * 16);
    auto load_frags = [&](int slot, int ks) {
        const int64_t o = (int64_t)min(ks, NKS - 1) * NT * 2048;
        mh[slot] = *(gh8 *)(tbase + o);
        ml[slot] = *(gh8 *)(tbase + o + 1024);
        if constexpr (MARG) {
            ch[slot] = *(gh8 *)(cbase + o);
            cl[slot] = *(gh8 *)(cbase + o + 1024);
        }
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) load_frags(k, k);
    static_assert((MARG ? 4 : 2) * PF == 24, "the counted wait below");
    // The wave's own K-steps of the tile have landed once only the 24 fragment loads behind them are outstanding (hipcc
    // does not count the asm DMAs, and they are older than every load it does count).
    asm volatile("s_waitcnt vmcnt(24)" ::: "memory");

    // ---- phase 0: f32 -> f16 pairs, in place, ONCE per tile -----------------------------------------------------------
    // Every wave multiplies the same x tile: converting in the K loop was 45 VALU instructions per K-step in each of the
    // 8 waves.  Here a wave converts the K-steps it fetched itself: the 32 bytes lane (s, h) would read as 8 floats become
    // [8 x f16 high | 8 x f16 low], the two B operands of its MFMAs.  With the conversion go the bookkeeping of the
    // K-step (sum x^2, NaN / out-of-range values -> 0 with the K-step flagged; a NaN leaves a NaN low half as its mark,
    // which a finite residual never is) -- per wave, combined through the LDS tail after the barrier.
    const int sw = (s >> 2) & 3;
    const unsigned xo0 = (unsigned)(s * 64 + (((h * 2) ^ sw) << 4)), xo1 = (unsigned)(s * 64 + (((h * 2 + 1) ^ sw) << 4));
    ltail *tail = (ltail *)(smem + NKS * 2048 + kWideWaves * 2 * S * I * I * 4);
    {
        float qsum = 0.f;
        bool need_exact = false, saw_nan = false;
        unsigned long long odd_part = 0ull;
        for (int ks = wave; ks < NKS; ks += kWideWaves) {
            lchar *xb = smem + ks * 2048;
            const gf32x4 x0 = *(lf4 *)(xb + xo0), x1 = *(lf4 *)(xb + xo1);
            float v[8];
            {
                const int f0 = ks * 16 + h * 8;
                const bool in0 = f0 + 4 <= D, in1 = f0 + 8 <= D;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = in0 ? x0[i] : 0.f;
                    v[4 + i] = in1 ? x1[i] : 0.f;
                }
            }
            gf32x2 tq2 = {0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                const gf32x2 pv = {v[i], v[i + 1]};
                tq2 = __builtin_elementwise_fma(pv, pv, tq2);
            }
            float tq = tq2[0] + tq2[1];
            const bool bad = !(tq < kGemmStepBound);
            unsigned nanm = 0u;
            if (__any(bad)) odd_part |= 1ull << ks;
            if (bad) {
                tq = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float vi = v[i];
                    const bool isn = vi != vi;
                    const bool big = !isn && !(fabsf(vi) < kGemmAbsBound);
                    need_exact = need_exact || big;
                    saw_nan = saw_nan || isn;
                    nanm |= isn ? (1u << i) : 0u;
                    v[i] = (isn || big) ? 0.f : vi;
                    tq = fmaf(v[i], v[i], tq);
                }
            }
            qsum += tq;
            half8 xh, xl;
            split8(v, xh, xl);
            if (bad) {
                u16x8 lb = __builtin_bit_cast(u16x8, xl);
#pragma unroll
                for (int i = 0; i < 8; ++i) lb[i] = ((nanm >> i) & 1u) ? kWideNanMark : lb[i];
                xl = __builtin_bit_cast(half8, lb);
            }
            *(lh8 *)(xb + xo0) = xh;
            *(lh8 *)(xb + xo1) = xl;
        }
        tail->qpart[wave][lane] = qsum;
        need_exact = __any(need_exact);
        saw_nan = __any(saw_nan);
        if (lane == 0) {
            tail->odd[wave] = odd_part;
            tail->flags[wave] = (need_exact ? 1 : 0) | (saw_nan ? 2 : 0);
        }
    }
    // the wave's sum weights (linear softmax rows of its two partitions) into its LDS slice
    {
        const float *wp = a.W0 + (int64_t)rho * 2 * S * I * I;
        for (int e = lane; e < 2 * S * I * I; e += 64) w0_l[e] = wp[e];
    }
    bool model_ok = a.elig[min(lane, NT - 1)] != 0;   // (every repetition's verdict: the root adds one common term)
    __syncthreads();   // the converted tile and the waves' shares of its bookkeeping are in LDS for everyone

    unsigned long long odd_mask = 0ull;   // K-steps whose constants the validity GEMM accumulates
    float qtot = 0.f;
    int tflags = 0;
#pragma unroll
    for (int w = 0; w < kWideWaves; ++w) {
        odd_mask |= tail->odd[w];
        qtot += tail->qpart[w][lane];
        tflags |= tail->flags[w];
    }
    odd_mask = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(odd_mask >> 32)) << 32) |
               (unsigned)__builtin_amdgcn_readfirstlane((int)odd_mask);
    tflags = __builtin_amdgcn_readfirstlane(tflags);
    qtot += __shfl_xor(qtot, 32, 64);
    const bool need_exact = (tflags & 1) != 0, saw_nan = (tflags & 2) != 0;

    // ---- phase 1: P^T = M^T x^T over the whole K range of the wave's tile --------------------------------------------
    gf32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    // One K-step of the wave's tile against the fragments in slot k (a constant in every unrolled copy): two LDS reads,
    // three MFMAs; a flagged K-step (wave-uniform, no memory operation behind the branch) takes its validity operand from
    // the NaN marks and, in the build for marginalised evidence, multiplies it with the constants in flight.
    auto kstep = [&](int k, int ks) __attribute__((always_inline)) {
        const lchar *xb = smem + ks * 2048;
        const half8 xh = *(const lh8 *)(xb + xo0);
        half8 xl = *(const lh8 *)(xb + xo1);
        const bool odd = (odd_mask >> ks) & 1ull;
        half8 valid;
        if (odd) {
            u16x8 lb = __builtin_bit_cast(u16x8, xl);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool isn = lb[i] == kWideNanMark;
                valid[i] = isn ? (_Float16)0.0f : (_Float16)1.0f;
                lb[i] = isn ? (unsigned short)0 : lb[i];
            }
            xl = __builtin_bit_cast(half8, lb);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[k], xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[k], xl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml[k], xh, acc, 0, 0, 0);
        if constexpr (MARG) {
            if (odd) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ch[k], valid, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cl[k], valid, acc, 0, 0, 0);
            }
        }
    };
    // (a.ablate: measurement only, DPK_GEMM_ABLATE -- 1 no K loop, 2 no upper layers)
    // Whole groups of PF K-steps first: straight-line code, the fragment loads unconditional (a load behind a branch makes
    // hipcc wait for ALL outstanding loads at the join).  The row's last K-steps after them, without prefetch.
    int k0 = 0;
    unsigned long long peeked = 0ull;     // the launch's verdict word as of the last full group of K-steps (np > 0)
    if (compute && !(a.ablate & 1)) {
        for (; k0 + PF <= NKS; k0 += PF) {
            peeked = vi_peek(pa.ctl);      // (unconditional, every thread, one request per wave: the last group's is the one used)
#pragma unroll
            for (int k = 0; k < PF; ++k) {
                kstep(k, k0 + k);
                load_frags(k, k0 + k + PF);   // (the slot is free again: the fragments PF K-steps ahead)
            }
        }
#pragma unroll
        for (int k = 0; k < PF - 1; ++k)
            if (k0 + k < NKS) kstep(k, k0 + k);   // (wave-uniform)
    }
    if constexpr (!MARG) {
        // Flagged K-steps of the clean build: their validity GEMM, from the tile still in LDS (out of the loop above: its
        // constants are loaded on demand).
        for (int ks = 0; ks < (compute ? NKS : 0); ++ks) {
            if (!((odd_mask >> ks) & 1ull)) continue;   // (wave-uniform)
            const u16x8 lb = __builtin_bit_cast(u16x8, *(const lh8 *)(smem + ks * 2048 + xo1));
            half8 valid;
#pragma unroll
            for (int i = 0; i < 8; ++i) valid[i] = (lb[i] == kWideNanMark) ? (_Float16)0.0f : (_Float16)1.0f;
            const int64_t o = (int64_t)ks * NT * 2048;
            const half8 c0 = *(gh8 *)(cbase + o), c1 = *(gh8 *)(cbase + o + 1024);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c0, valid, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(c1, valid, acc, 0, 0, 0);
        }
    }
    // the expanded square is within the 1e-5 bar while sum x^2 <= 36 D (|mu| <= 6: DESIGN 3.3)
    const bool lane_exact = need_exact || !(qtot <= kExpandBound * kExpandBound * (float)D);
    model_ok = __all(model_ok);
    WideUpFrags<S> uf;
    uf.load(a, rho, lane);      // (in flight under the MFMA tail, the verdict and the barrier)
    // the launch's verdict on its tables (np > 0): published long ago by the table work-groups -- one L2 round trip for
    // thread 0 under the other waves' K loops; the barrier below hands it to everyone
    unsigned vi_ticket = 0u;
    if (np > 0 && tid == 0) {
        tail->verdict = vi_verdict(pa.ctl, np, peeked) ? 1 : 0;
        // (the reader ticket: requested now, looked at when the work-group leaves -- nothing in between waits for it)
        vi_ticket = __hip_atomic_fetch_add(&pa.ctl->readers, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    __syncthreads();   // every wave is done with the x tile: its LDS becomes scratch and the root exchange buffer
    const bool tables_stale = np > 0 && tail->verdict != 0;
    const bool exact = !model_ok || __any(lane_exact) || tables_stale;   // (the same x tile in every wave: the same verdict in every wave)
    double part = wide_block_upper<S, true, EMIT, NW>(a, acc, odd_mask, qtot, exact, rho, mine, b0, w0_l, smem_generic, uf,
                                      tables_stale ? pa.w[0] : nullptr, tables_stale ? pa.w[1] : nullptr,
                                      NW == kWideWaves ? nullptr : pa.wx_part + (int64_t)blk * 2 * 32 * a.C * 2,
                                      NW == kWideWaves ? nullptr : pa.wx_tick + blk, grp);
    double *red = reinterpret_cast<double *>(smem_generic + wide_upper_lds_bytes(NT, a.C));
    if (a.ll_sum != nullptr) {
        part = wave_reduce_sum(part);
        __syncthreads();
        if (lane == 0) red[wave] = part;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
#pragma unroll
            for (int w = 0; w < kWideWaves; ++w) tot += red[w];
            atomicAdd(a.ll_sum + (a.ll_cnt > 1 ? ((int)blockIdx.x & 15) : 0), tot);
            if ((int)blockIdx.x == np) atomicAdd(a.ll_sum + a.ll_cnt, (double)a.B * (double)a.C);
        }
    }
    if (saw_nan && tid == 0 && a.slow_flag != nullptr) *a.slow_flag = a.launch_seq;
    if (np > 0 && tid == 0) vi_done(pa.ctl, vi_ticket, pa.readers);
}

// ------------------------------------------------------------------------------------------------
// large batches: 128-sample tiles, x through a three-stage LDS-DMA ring, converted once per tile
// ------------------------------------------------------------------------------------------------
// The 32-sample kernel above re-reads the repetition's table fragments (98 KB per wave, 784 KB per work-group) for every
// 32 samples -- 27.6 KB of L2 -> CU traffic per sample, which bounds it -- and every one of its 8 waves converts the SAME
// x values to f16 pairs (45 VALU instructions against 3 MFMAs per K-step).  Here
//   * a compute wave (= repetition) keeps FOUR 32-sample blocks in flight against each fragment (64 accumulator
//     registers): 6.9 KB of table traffic per sample;
//   * 128 rows of x do not fit LDS next to the scratch, so x arrives in 64-feature chunks through a ring of three 32 KB
//     stages (the row layout of the 2-channel ring: 256-byte rows of sixteen 16-byte pieces, XOR-swizzled by row & 15 on
//     the source side).  Waves 8-11 are the loader waves, one per sample block: a loader wave DMAs its block's 32 rows
//     of the chunk, waits for them (counted vmcnt), and converts them IN PLACE -- the 32 bytes a lane read as 8 floats
//     become [8 x f16 high | 8 x f16 low], exactly the two B operands the MFMAs take -- before the chunk's barrier.  It
//     also does the per-chunk bookkeeping once instead of eight times: sum x^2 per row, the K-steps that hold NaN / out of
//     range values (flags per block and K-step; such a value counts as 0 in the product),
//     the block's exact-evaluation verdict;
//   * the compute waves' K loop is then two 16-byte LDS reads and three MFMAs per block and K-step.
// One tile per work-group: the upper part needs work-group barriers, which a ring running on across tile boundaries could
// not share with the loaders.
constexpr int kWideRingBlocks = 4;
struct WideRingTail {                                 // LDS behind the ring's stages
    unsigned flags[kGemmStages][kWideRingBlocks];     // per stage and block: bit k = K-step k of the chunk needs the validity GEMM
    float qrow[kGemmTile];                            // sum x^2 per row of the tile (finite, in-range values)
    int exact[kWideRingBlocks];                       // the block leaves the expanded form
    int saw_nan;
    int pad[3];
};
static_assert(sizeof(WideRingTail) % 16 == 0, "the waves' weight slices follow");

template <int S>
__global__ __launch_bounds__((kWideWaves + kGemmWaves) * 64) void ratspn_gemm_wide_ring_kernel(const GemmArgs a) {
    constexpr int NB = kWideRingBlocks;
    constexpr int KS = 4, KC = 16 * KS, ROWB = KC * 4, STAGE = kGemmTile * ROWB, NS = kGemmStages;
    constexpr int PX = 8;                              // DMA instructions per loader wave and chunk (4 rows each)
    constexpr int PF = KS;                             // K-steps of table fragments in flight (one chunk: 168 VGPRs at 12 waves)
    typedef const __attribute__((address_space(1))) half8 gh8;
    typedef __attribute__((address_space(3))) gf32x4 lf4;
    typedef __attribute__((address_space(3))) half8 lh8;
    typedef __attribute__((address_space(3))) WideRingTail ltail;
    static_assert(kGemmTile == 32 * NB && kGemmWaves == NB && NS == 3, "one loader wave per block; counted waits");

    extern __shared__ __attribute__((aligned(16))) char smem_generic[];
    lchar *smem = (lchar *)smem_generic;
    ltail *tail = (ltail *)(smem + NS * STAGE);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave12 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D, NT = a.reps, NCH = (D + KC - 1) / KC;
    const int NKS = (D + 15) >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * kGemmTile;
    if (tid == 0) tail->saw_nan = 0;

    if (wave12 >= kWideWaves) {
        // ================= loader wave w: rows [32 w, 32 w + 32) of the tile = sample block w ==========================
        const int w = wave12 - kWideWaves;
        __builtin_amdgcn_s_setprio(3);                 // (the chunk's barrier waits for this wave's conversion: first in line at issue)
        const int nvalid = (int)min((int64_t)kGemmTile, a.B - t0);
        const gcchar_p xt = (gcchar_p)(a.x + t0 * D);
        const unsigned smem_base = (unsigned)(uintptr_t)smem;
        unsigned voff[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int rl = w * 32 + j * 4 + (lane >> 4);
            voff[j] = (unsigned)(min(rl, nvalid - 1) * D + (((lane & 15) ^ (rl & 15)) << 2)) * 4u;
        }
        auto issue = [&](int pc) {
            const unsigned st = smem_base + (pc % NS) * STAGE + w * 32 * ROWB;
            if ((pc + 1) * KC <= D) {
#pragma unroll
                for (int j = 0; j < PX; ++j) glds16(voff[j] + pc * (KC * 4), xt, st + j * 4 * ROWB);
            } else {   // last chunk of a ragged row: pieces beyond it re-fetch the last one (zeroed by the conversion)
                const int vp = (D - pc * KC) >> 2;
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    const int rl = w * 32 + j * 4 + (lane >> 4);
                    const int gp = min((lane & 15) ^ (rl & 15), vp - 1);
                    glds16((unsigned)(min(rl, nvalid - 1) * D + pc * KC + gp * 4) * 4u, xt, st + j * 4 * ROWB);
                }
            }
        };
        // the lane's share of a chunk: K-step (lane & 7) >> 1, feature half lane & 1 of the rows j * 8 + (lane >> 3)
        const int ks4 = (lane & 7) >> 1, h = lane & 1, pcs = ks4 * 4 + h * 2;
        float qacc[4] = {0.f, 0.f, 0.f, 0.f};
        bool need_exact = false, saw_nan = false;
        auto convert = [&](int pc) {
            lchar *st = smem + (pc % NS) * STAGE;
            const int f0 = (pc * KS + ks4) * 16 + h * 8;
            const bool in0 = f0 + 4 <= D, in1 = f0 + 8 <= D;
            unsigned long long bad_lanes = 0ull;
            gf32x4 xa[4], xb[4];                       // (all eight reads first: one LDS round trip per chunk, not four)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rl = w * 32 + j * 8 + (lane >> 3), sw = rl & 15;
                xa[j] = *(lf4 *)(st + rl * ROWB + ((pcs ^ sw) << 4));
                xb[j] = *(lf4 *)(st + rl * ROWB + (((pcs | 1) ^ sw) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rl = w * 32 + j * 8 + (lane >> 3), sw = rl & 15;
                lchar *p0 = st + rl * ROWB + ((pcs ^ sw) << 4), *p1 = st + rl * ROWB + (((pcs | 1) ^ sw) << 4);
                const gf32x4 x0 = xa[j], x1 = xb[j];
                float v[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = in0 ? x0[i] : 0.f;
                    v[4 + i] = in1 ? x1[i] : 0.f;
                }
                gf32x2 tq2 = {0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    const gf32x2 pv = {v[i], v[i + 1]};
                    tq2 = __builtin_elementwise_fma(pv, pv, tq2);
                }
                float tq = tq2[0] + tq2[1];
                const bool bad = !(tq < kGemmStepBound);
                bad_lanes |= __ballot(bad);
                if (bad) {   // (a NaN or an out-of-range value counts as 0 here; the compute waves add the K-step's validity GEMM)
                    tq = 0.f;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float vi = v[i];
                        const bool isn = vi != vi;
                        const bool big = !isn && !(fabsf(vi) < kGemmAbsBound);
                        need_exact = need_exact || big;
                        saw_nan = saw_nan || isn;
                        v[i] = (isn || big) ? 0.f : vi;
                        tq = fmaf(v[i], v[i], tq);
                    }
                }
                qacc[j] += tq;
                half8 xh, xl;
                split8(v, xh, xl);
                *(lh8 *)p0 = xh;
                *(lh8 *)p1 = xl;
            }
            if (lane == 0) {
                unsigned fl = 0u;
#pragma unroll
                for (int k = 0; k < KS; ++k) fl |= (bad_lanes & (0x0303030303030303ull << (2 * k))) ? (1u << k) : 0u;
                tail->flags[pc % NS][w] = fl;
            }
        };
        issue(0);
        if (NCH > 1) issue(1);
        __syncthreads();   // (the compute waves fill their constants meanwhile)
        for (int c = 0; c < NCH; ++c) {
            // this wave's rows of chunk c have landed once at most one later chunk is still in flight
            if (c + 1 < NCH) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PX) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (!(a.ablate & 4)) convert(c);
            gemm_lds_barrier();   // chunk c is converted for everyone; everyone is done reading chunk c - 1
            if (c + 2 < NCH) issue(c + 2);
        }
        // the tile's sums: 8 lanes hold a row's K-step / half shares
        bool blk_exact = need_exact;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float q = qacc[j];
            q += __shfl_xor(q, 1, 64);
            q += __shfl_xor(q, 2, 64);
            q += __shfl_xor(q, 4, 64);
            if ((lane & 7) == 0) tail->qrow[w * 32 + j * 8 + (lane >> 3)] = q;
            // the expanded square is within the 1e-5 bar while sum x^2 <= 36 D (|mu| <= 6: DESIGN 3.3)
            blk_exact = blk_exact || !(q <= kExpandBound * kExpandBound * (float)D);
        }
        blk_exact = __any(blk_exact);
        if (lane == 0) tail->exact[w] = blk_exact ? 1 : 0;
        if (__any(saw_nan) && lane == 0) tail->saw_nan = 1;
        __syncthreads();                               // (the compute waves' "ring is idle" barrier)
        for (int blk = 0; blk < NB; ++blk) wide_upper_barriers();
        if (a.ll_sum != nullptr) {
            __syncthreads();
            __syncthreads();
        }
        return;
    }
    // ===================== compute wave = repetition ======================================================================
    const int wave = wave12;
    const int s = lane & 31, h = lane >> 5;
    const bool mine = wave < NT;
    const int rho = mine ? wave : NT - 1;
    half8 mh[PF], ml[PF];
    const gcchar_p tbase = (gcchar_p)a.mtab + ((int64_t)rho * 2048 + lane * 16);
    const gcchar_p cbase = (gcchar_p)a.ctab + ((int64_t)rho * 2048 + lane * 16);
    auto load_frags = [&](int slot, int ks) {
        const int64_t o = (int64_t)min(ks, NKS - 1) * NT * 2048;
        mh[slot] = *(gh8 *)(tbase + o);
        ml[slot] = *(gh8 *)(tbase + o + 1024);
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) load_frags(k, k);
    lfloat *w0_l = (lfloat *)(smem + NS * STAGE + sizeof(WideRingTail)) + wave * (2 * S * kWideI * kWideI);
    {
        const float *wp = a.W0 + (int64_t)rho * 2 * S * kWideI * kWideI;
        for (int e = lane; e < 2 * S * kWideI * kWideI; e += 64) w0_l[e] = wp[e];
    }
    bool model_ok = a.elig[min(lane, NT - 1)] != 0;   // (every repetition's verdict: the root adds one common term)
    __syncthreads();   // (pairs with the loaders' opening one)

    gf32x16 acc[NB];
    unsigned long long odd_mask[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
        odd_mask[q] = 0ull;
    }
    // The hot loop is straight-line code -- two LDS reads and three MFMAs per block and K-step, the fragments one chunk
    // ahead -- with nothing conditional that touches a memory counter: a branch with a load behind it makes hipcc's
    // counter bookkeeping give up at the join (vmcnt(1) in front of every K-step: the L2 latency of the fragment just
    // requested, 20 us per tile).  Hence K-steps with flagged values only leave a bit here and are finished below.
    auto chunk = [&](auto nk_c, int c, int cstage) {
        constexpr int NK = decltype(nk_c)::value;
        gemm_lds_barrier();   // the loaders have converted this chunk; everyone is done with the previous one
        const lchar *st = smem + cstage * STAGE;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const unsigned fl = (unsigned)__builtin_amdgcn_readfirstlane((int)tail->flags[cstage][q]);
            odd_mask[q] |= (unsigned long long)fl << (c * KS);
        }
        // (block, K-step) pairs in sequence, the operands of the pair two ahead requested before each MFMA group; the
        // scheduling barriers keep hipcc from hoisting all 32 reads of the chunk (128 registers) to the top
        if (a.ablate & 1) return;
        constexpr int NP = NK * NB, AHEAD = 2;
        half8 xh[AHEAD + 1], xl[AHEAD + 1];
        auto request = [&](int n, half8 &dh, half8 &dl) {
            const int kk = n / NB, q = n % NB;
            const int rl = q * 32 + s, sw = rl & 15, pcs = kk * 4 + h * 2;
            dh = *(const lh8 *)(st + rl * ROWB + ((pcs ^ sw) << 4));
            dl = *(const lh8 *)(st + rl * ROWB + (((pcs | 1) ^ sw) << 4));
        };
#pragma unroll
        for (int n = 0; n < AHEAD && n < NP; ++n) request(n, xh[n], xl[n]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            const int kk = n / NB, q = n % NB, cur = n % (AHEAD + 1);
            if (n + AHEAD < NP) request(n + AHEAD, xh[(n + AHEAD) % (AHEAD + 1)], xl[(n + AHEAD) % (AHEAD + 1)]);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[kk], xh[cur], acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[kk], xl[cur], acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml[kk], xh[cur], acc[q], 0, 0, 0);
            if (q == NB - 1) load_frags(kk, c * KS + kk + PF);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    const int NCHF = NKS / KS, NKT = NKS - NCHF * KS;   // full chunks, K-steps of the last one
    int cstage = 0;
    for (int c = 0; c < NCHF; ++c) {
        chunk(std::integral_constant<int, KS>(), c, cstage);
        cstage = (cstage + 1 == NS) ? 0 : cstage + 1;
    }
    if (NKT > 0) {   // the row's last, partial chunk (once per tile: plain code)
        gemm_lds_barrier();
        const lchar *st = smem + cstage * STAGE;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const unsigned fl = (unsigned)__builtin_amdgcn_readfirstlane((int)tail->flags[cstage][q]);
            odd_mask[q] |= (unsigned long long)fl << (NCHF * KS);
        }
#pragma unroll
        for (int kk = 0; kk < KS - 1; ++kk) {
            if (kk < NKT) {
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    const int rl = q * 32 + s, sw = rl & 15, pcs = kk * 4 + h * 2;
                    const half8 xh = *(const lh8 *)(st + rl * ROWB + ((pcs ^ sw) << 4));
                    const half8 xl = *(const lh8 *)(st + rl * ROWB + (((pcs | 1) ^ sw) << 4));
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[kk], xh, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(mh[kk], xl, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ml[kk], xh, acc[q], 0, 0, 0);
                }
            }
        }
    }
    // flagged K-steps (NaN or out-of-range values, counted as 0 above): the constants of the features that ARE present,
    // as a validity GEMM from x as it lies in global memory.  (On demand: a launch that keeps meeting NaN takes the
    // 32-sample kernel's build with both tables in flight.)
#pragma unroll
    for (int q = 0; q < NB; ++q) {
        if (odd_mask[q] == 0ull) continue;   // (wave-uniform)
        const float *xr = a.x + min(t0 + q * 32 + s, a.B - 1) * D;
        for (int ks = 0; ks < NKS; ++ks) {
            if (!((odd_mask[q] >> ks) & 1ull)) continue;
            const int f0 = ks * 16 + h * 8;
            half8 valid;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float vi = (f0 + i < D) ? xr[f0 + i] : 0.f;
                valid[i] = (vi != vi) ? (_Float16)0.0f : (_Float16)1.0f;
            }
            const int64_t o = (int64_t)ks * NT * 2048;
            const half8 c0 = *(gh8 *)(cbase + o), c1 = *(gh8 *)(cbase + o + 1024);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(c0, valid, acc[q], 0, 0, 0);
            acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(c1, valid, acc[q], 0, 0, 0);
        }
    }
    model_ok = __all(model_ok);
    WideUpFrags<S> uf{};        // (unused: the ring kernel fetches the fragments tile by tile inside the upper part)
    __syncthreads();   // the ring is idle: its stages become scratch and the root exchange buffer; the tail is complete
    // (Measured and dropped, round 3: the two halves of a wave trading partitions across two blocks so that the sum weights
    // are wave-uniform and come through the scalar cache instead of LDS -- 63 us per tile against 54: 32 KB of weights per
    // work-group do not stay in the 16 KB scalar cache, and every s_load_dwordx16 then waits for the L2.)
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < NB; ++q)
        part += wide_block_upper<S, false>(a, acc[q], odd_mask[q], tail->qrow[q * 32 + s], !model_ok || tail->exact[q] != 0, rho, mine,
                                    t0 + q * 32, w0_l, smem_generic, uf);
    if (a.ll_sum != nullptr) {
        double *red = reinterpret_cast<double *>(smem_generic + wide_upper_lds_bytes(NT, a.C));
        part = wave_reduce_sum(part);
        __syncthreads();
        if (lane == 0) red[wave] = part;
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
#pragma unroll
            for (int w = 0; w < kWideWaves; ++w) tot += red[w];
            atomicAdd(a.ll_sum + (a.ll_cnt > 1 ? ((int)blockIdx.x & 15) : 0), tot);
            if (blockIdx.x == 0) atomicAdd(a.ll_sum + a.ll_cnt, (double)a.B * (double)a.C);
        }
    }
    if (tid == 0 && tail->saw_nan != 0 && a.slow_flag != nullptr) *a.slow_flag = a.launch_seq;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
bool gemm_wide_shape_ok(int D, int reps, int I, int S, int C) {
    if (I != kWideI || !(S == 2 || S == 4 || S == 8) || reps < 1 || reps > kWideWaves || C > kWideMaxC) return false;
    const int NKS = cdiv(D, 16);
    if (NKS > 64) return false;   // K-step bit mask
    // LDS: the x tile + the waves' sum weights; afterwards scratch (32 KB) + the root exchange buffer in its place
    const size_t p1 = (size_t)NKS * 2048 + (size_t)kWideWaves * 2 * S * kWideI * kWideI * 4 + sizeof(WideTail);
    const size_t p2 = (size_t)kWideWaves * 64 * 2 * kWideI * 4 + ((size_t)reps * 32 * C * 2 + 32) * 4 + kWideWaves * 8 + 64;
    return p1 <= 160 * 1024 && p2 <= (size_t)NKS * 2048;
}

// two work-groups per block (NW = 4) while that still fits one round of the chip and the model has repetitions for both
static bool wide_splits_blocks(const GemmArgs &a, const GemmPrepArgs &p) {
    static const int mode = [] { const char *e = getenv("DPK_WIDE_SPLIT"); return e ? atoi(e) : -1; }();   // (0 / 1: A/B runs)
    const int64_t blocks = cdiv(a.B, 32);
    if (p.wx_part == nullptr || a.reps <= 4 || blocks > kWideSplitBlocks) return false;
    if (mode >= 0) return mode != 0;
    return 2 * blocks + p.np <= device_cus();
}

template <int S, bool MARG, bool EMIT, int NW>
static int gemm_wide_launch_nw(const GemmArgs &a, const GemmPrepArgs &p, hipStream_t st) {
    const int NKS = cdiv(a.D, 16);
    size_t lds = (size_t)NKS * 2048 + (size_t)kWideWaves * 2 * S * kWideI * kWideI * 4 + sizeof(WideTail);
    if (p.np > 0 && gemm_prep_lds_bytes(a.D, kWideI, a.d) > lds) lds = gemm_prep_lds_bytes(a.D, kWideI, a.d);
    auto kern = ratspn_gemm_wide_kernel<S, MARG, EMIT, NW>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), 160 * 1024)) return rc;
    Profile prof(DPK_KERNEL_RATSPN_FUSED, st);
    GemmPrepArgs pp = p;
    const int blocks = (int)cdiv(a.B, 32);
    const int model_wgs = NW == kWideWaves ? blocks : 2 * (int)align_up(blocks, 8);   // (NW = 4: whole groups of 16, see the kernel)
    pp.readers = p.np + (NW == kWideWaves ? blocks : 2 * blocks);
    DPK_LAUNCH_IN(prof, "ratspn_gemm_wide_kernel", kern, dim3(p.np + model_wgs), dim3(kWideWaves * 64), lds, st, a, pp);
    return DPK_OK;
}
template <int S, bool MARG, bool EMIT = false>
static int gemm_wide_launch(const GemmArgs &a, const GemmPrepArgs &p, hipStream_t st) {
    if (wide_splits_blocks(a, p)) return gemm_wide_launch_nw<S, MARG, EMIT, 4>(a, p, st);
    return gemm_wide_launch_nw<S, MARG, EMIT, kWideWaves>(a, p, st);
}

template <int S>
static int gemm_wide_ring_launch(const GemmArgs &a, hipStream_t st) {
    const size_t lds = (size_t)kGemmStages * kGemmTile * 256 + sizeof(WideRingTail) + (size_t)kWideWaves * 2 * S * kWideI * kWideI * 4;
    auto kern = ratspn_gemm_wide_ring_kernel<S>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), 160 * 1024)) return rc;
    Profile prof(DPK_KERNEL_RATSPN_FUSED, st);
    DPK_LAUNCH_IN(prof, "ratspn_gemm_wide_ring_kernel", kern, dim3(cdiv(a.B, kGemmTile)),
                  dim3((kWideWaves + kGemmWaves) * 64), lds, st, a);
    return DPK_OK;
}

// The 128-sample ring kernel is taken above a multiple of the small-batch threshold (dpk_ratspn_small_batch_max: 0 = ring
// kernels always, which is how the tests reach it at every batch size); DPK_WIDE_RING_MIN overrides for measurements.
constexpr int kWideRingFactor = 1;
int64_t gemm_small_max_batch();   // ratspn_gemm_small.hip
static bool wide_takes_ring(int64_t B) {
    static const int64_t forced = [] {
        const char *e = getenv("DPK_WIDE_RING_MIN");
        return e ? (int64_t)atoll(e) : (int64_t)-1;
    }();
    return forced >= 0 ? B >= forced : B > gemm_small_max_batch() * kWideRingFactor;
}

// large clean batches: 128-sample tiles behind the LDS-DMA ring (its scratch must fit the ring's stages); everything else
// takes the 32-sample kernel -- the mapping that carries its own table work-groups (ratspn_gemm_forward asks)
bool gemm_wide_takes_tile32(int64_t B, int D, int reps, int C, bool marginal, bool emit) {
    if (emit) return true;   // (the training forward lives in the 32-sample kernel only)
    return !(!marginal && wide_takes_ring(B) && (D % 4) == 0 &&
             wide_upper_lds_bytes(reps, C) + kWideWaves * 8 + 64 <= (size_t)kGemmStages * kGemmTile * 256);
}

// The caller (ratspn_gemm_forward) has built the tables (or handed their check to this launch: p.np > 0, 32-sample kernel
// only) and filled the argument block.
int ratspn_gemm_wide_forward(const GemmArgs &a, const GemmPrepArgs &p, int S, hipStream_t st) {
    const bool marg = a.marginal != 0;
    if (a.emit_leaf != nullptr) {
        switch (S) {
            case 2: return marg ? gemm_wide_launch<2, true, true>(a, p, st) : gemm_wide_launch<2, false, true>(a, p, st);
            case 4: return marg ? gemm_wide_launch<4, true, true>(a, p, st) : gemm_wide_launch<4, false, true>(a, p, st);
            case 8: return marg ? gemm_wide_launch<8, true, true>(a, p, st) : gemm_wide_launch<8, false, true>(a, p, st);
        }
        set_error("ratspn_gemm_wide: sums=%d not built", S);
        return DPK_EUNSUPPORTED;
    }
    if (!gemm_wide_takes_tile32(a.B, a.D, a.reps, a.C, marg, false)) {
        DPK_REQUIRE(p.np == 0, DPK_EINVAL, "ratspn_gemm_wide: the ring kernel does not check its tables itself");
        switch (S) {
            case 2: return gemm_wide_ring_launch<2>(a, st);
            case 4: return gemm_wide_ring_launch<4>(a, st);
            case 8: return gemm_wide_ring_launch<8>(a, st);
        }
    }
    switch (S) {
        case 2: return marg ? gemm_wide_launch<2, true>(a, p, st) : gemm_wide_launch<2, false>(a, p, st);
        case 4: return marg ? gemm_wide_launch<4, true>(a, p, st) : gemm_wide_launch<4, false>(a, p, st);
        case 8: return marg ? gemm_wide_launch<8, true>(a, p, st) : gemm_wide_launch<8, false>(a, p, st);
    }
    set_error("ratspn_gemm_wide: sums=%d not built", S);
    return DPK_EUNSUPPORTED;
}

}  // namespace dpk
