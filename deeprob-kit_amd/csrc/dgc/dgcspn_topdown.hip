// Top-down pass of a DGC-SPN in ONE launch: DgcSpn.sample (mode 1), DgcSpn.sample_conditional (mode 2) and
// DgcSpn.mpe_completion (mode 3).
//
// reference: deeprob/spn/models/dgcspn.py raises NotImplementedError in `sample` and has no conditional sampler; the
// circuit is the one its forward evaluates (SpatialGaussianLayer, SpatialProductLayer, SpatialSumLayer, SpatialRootLayer of
// deeprob/spn/layers/dgcspn.py).  Every root input (c, h, w) is a product that reaches every pixel at most once through the
// dilated 2x2 windows, so an ancestral draw is well defined; it needs one chosen-channel-or-none map per level.
//
// The pass.  Inputs, all fp32 NCHW on the device: the evidence x [B, C, H, W] (NaN = to be drawn; null = everything is
// drawn), act[0] = the leaf layer's output [B, K, H, W], act[t] = the output of the t-th SpatialSumLayer, logw[t] = the
// log_softmax(weight, 1) of that sum layer, the root's log_softmax(weight, 1) [classes, Cr Hr Wr], y [B] int64 (null =
// class 0), the leaf loc / scale [K, C, H, W], and the geometry of every product level j = 0 .. L-1 (in and out shape, the
// four pads, stride, dilation, the depthwise flag; include/deeprob_dgc.h).  Sum layer t sits on product level t - 1.
//
// Product maps are never materialised.  A product value is formed where it is needed as the fp32 sum of its four taps in
// row-major tap order (th, tw): ((v0 + v1) + v2) + v3.
//   - The input coordinate of a tap is out * stride + t * dilation - pad_before.
//   - A tap outside [0, in) contributes 0 and has no child.
//   - A depthwise level reads channel oc at every tap; any other level decodes the output channel in itertools.product
//     order: tap t = 2 th + tw gets digit (oc / Cin^(3 - t)) % Cin.
//
// Per sample, top to bottom:
//   Root.  s(i) = prod_value_{L-1}(i) + logw_root[y, i] for i over the flattened last product map (c, h, w).  One i is drawn
//     by inverse CDF over exp(s - max s) in index order.  It activates its taps: position (ih, iw) of the map of sum layer
//     L - 1 with the tap's channel.
//   Every sum layer t = L-1 .. 1.  Each active position (o, h, w) draws its input channel c by inverse CDF over
//     exp(s - max), s(c) = prod_value_{t-1}(c, h, w) + logw[t][o, c, h, w] (fp32, this operand order).
//     If the maximum is -inf or NaN the draw is by the bare weights, the inverse CDF over exp(logw) (step 3 of the RAT-SPN
//     definition, csrc/ratspn_topdown.hip).  The chosen product activates its taps with the decoded channels, in the map
//     of sum layer t - 1, or for t = 1 in the leaf map.
//   Leaves.  A pixel (h, w) reached with component k treats each of its C input channels separately: an observed entry is
//     copied bit for bit, a NaN entry is loc[k, c, h, w] + scale[k, c, h, w] * z with z = sqrt(-2 log(1 - u1)) cos(2 pi u2)
//     (Box-Muller from two counter-based uniforms, as in csrc/ratspn_topdown.hip).
//   Pixels out of scope.  A pixel that no path reaches (a 'valid' stride-2 level of an odd map drops its last row and column)
//     is returned as given: its evidence value, or NaN when everything is drawn; its entry of `choice` is -1.
//   Inverse CDF.  target = u * total, the first n with target < c(n) in index order, the last input when rounding leaves
//     none; total and c(n) are fp32 sums in index order (a node of more than 64 inputs:
//     dp_device::wave_inverse_cdf, in-order sums in contiguous lane chunks, then a scan over the lanes).
//   Draws.  u(ctr) = dp_device::counter_uniform(seed, ctr) (shared/device.h), ctr = row * slots_per_row + slot; slot 0 is the
//     root's, slot base_t + h * Wout_{t-1} + w that of sum layer t at (h, w) (base_1 = 1, base_{t+1} = base_t +
//     Hout_{t-1} Wout_{t-1}), slots base_L + 2 ((c H + h) W + w), + 1 the two uniforms of leaf entry (c, h, w).  A row's
//     output depends on (seed, row index, y) and its evidence only.
//   Mode 1 (no evidence) takes every activation as log 1: act == null, every draw is by the bare weights, no bottom-up pass.
//   Mode 3 (max-product completion) selects where mode 2 draws; arguments as in mode 2, `seed` is ignored and no uniform is
//     formed.  At the root and at every active position of every sum layer, with mode 2's scores s(n) (the same fp32
//     expressions, operand for operand) and their NaN-sticky maximum m: if m > -inf, the first n in index order with
//     s(n) == m; otherwise (m is -inf or NaN) the first n in index order that maximises logw(n), a NaN weight never over a
//     number -- the bare weights again.  Ties always go to the lowest index.  A node of more than 64 inputs: every lane
//     keeps the first maximum of its strided indices n = lane, lane + 64, ..., the wave then takes the largest value and
//     among equal values the smallest index.  Leaves: an observed entry is copied bit for bit, a NaN entry of a pixel
//     reached with component k is loc[k, c, h, w] bit for bit (the mode of a Gaussian); `scale` is not read.  The result is
//     the leaf modes of the induced tree chosen greedily from the sum-pass activations, as csrc/ratspn_topdown.hip's MPE.
//
// Shape of the kernel: one work-group of 256 threads per sample, grid-stride over samples.  The state between two levels is
// the list of the active positions of a map with their channels, (channel << 16 | position) -- the chosen-channel map in
// sparse form: an active node of a decomposable circuit owns at least one pixel, so a list never holds more than
// min(positions of the map, 4^(levels above)) entries.  Two lists ping-pong in LDS, appended to through one LDS counter per
// level (integer atomics; the order of a list does not matter: a node's draw depends on its own position's counter only),
// one barrier per level.  A node of at most 64 inputs is one lane's loop; a wider one (a non-depthwise level has Cin^4
// inputs, the root Cr Hr Wr) is scanned by a wave.  The scores are recomputed for every pass over them rather than kept:
// one sample's maps are a few KiB, hot in L1 / L2 after the first pass, and nothing is indexed dynamically in registers.
#include "dgc_common.h"
#include "../shared/device.h"
#include <algorithm>

namespace dpg_detail {

using dp_device::wave_inverse_cdf;
using dp_device::wave_max_nan;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWide = 64;            // a node of more inputs than this is scanned by a wave

struct TopDownArgs {
    int64_t B;
    int C, H, W, K, L, classes, cap;
    Level lv[DPG_MAX_LEVELS];
    const float *x;
    const int64_t *y;
    const float *act[DPG_MAX_LEVELS];
    const float *logw[DPG_MAX_LEVELS + 1];
    const float *loc, *scale;
    unsigned long long seed, slots;
    unsigned base[DPG_MAX_LEVELS + 1];   // [t], 1 <= t < L: first slot of sum layer t; [L]: first leaf slot
    float *out;
    int *choice;
};

// the taps of product (oc, oh, ow) inside the input map join the list of the level below
__device__ __forceinline__ void activate(const Level &g, int oc, int oh, int ow, int *list, int *count, int cap) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ih = oh * g.stride + (t >> 1) * g.dil - g.pt, iw = ow * g.stride + (t & 1) * g.dil - g.pl;
        if ((unsigned)ih < (unsigned)g.hin && (unsigned)iw < (unsigned)g.win) {
            const int k = atomicAdd(count, 1);
            // (k >= cap cannot happen in a decomposable circuit; a table that describes none must not write past the list)
            if (k < cap) list[k] = (tap_channel(g, oc, t) << 16) | (ih * g.win + iw);
        }
    }
}

// inverse CDF in index order over the non-negative weight(n) by one lane: dp_device::wave_inverse_cdf without the wave
template <typename WeightFn>
__device__ __forceinline__ int lane_inverse_cdf(int count, float u, WeightFn weight) {
    float total = 0.f;
    for (int n = 0; n < count; ++n) total += weight(n);
    const float target = u * total;
    float c = 0.f;
    for (int n = 0; n < count; ++n) {
        c += weight(n);
        if (target < c) return n;
    }
    return count - 1;
}

// First n in index order with value(n) == the NaN-sticky maximum of value, which is left in m; by one lane.  (A maximum of
// -inf or NaN: the caller does not use the index.)
template <typename ValueFn>
__device__ __forceinline__ int lane_first_max(int count, float &m, ValueFn value) {
    int at = 0;
    m = -INFINITY;
    for (int n = 0; n < count; ++n) {
        const float v = value(n);
        if (v > m) {
            m = v;
            at = n;
        } else if (v != v) {
            m = v;                                   // (once NaN, m stays NaN)
        }
    }
    return at;
}

// The same by a wave: every lane keeps the first maximum of its strided indices, then a butterfly takes the largest value
// and, among equal values, the smallest index.  Every lane ends with the same m and, when m is a number, the same index.
template <typename ValueFn>
__device__ __forceinline__ int wave_first_max(int count, int lane, float &m, ValueFn value) {
    int at = 0x7fffffff;
    m = -INFINITY;
    for (int n = lane; n < count; n += 64) {
        const float v = value(n);
        if (v > m) {
            m = v;
            at = n;
        } else if (v != v) {
            m = v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(m, o, 64);
        const int ta = __shfl_xor(at, o, 64);
        if (t > m || t != t || (t == m && ta < at)) {
            m = t;
            at = ta;
        }
    }
    return at == 0x7fffffff ? 0 : at;                // (no value above -inf: index 0, as the lane's loop)
}

// the number a weight counts as in mode 3's fallback: a NaN weight is never picked over a number
__device__ __forceinline__ float weight_or_least(float w) { return w != w ? -INFINITY : w; }

// the uniform of a node or leaf draw; mode 3 draws nothing and forms none
template <int MODE>
__device__ __forceinline__ float draw_uniform(unsigned long long seed, unsigned long long ctr) {
    return MODE == DPG_MODE_MPE ? 0.f : dp_device::counter_uniform(seed, ctr);
}

// One node's draw (mode 3: selection) among `count` inputs, by a wave (every lane returns the pick) or by one lane.
template <int MODE, typename ScoreFn, typename LogwFn>
__device__ __forceinline__ int wave_choose(int count, int lane, float u, ScoreFn score, LogwFn logw) {
    constexpr bool POSTERIOR = MODE == DPG_MODE_POSTERIOR;
    if (MODE == DPG_MODE_MPE) {
        float m;
        int at = wave_first_max(count, lane, m, score);
        // (wave-uniform; -inf and NaN: the bare weights.  All of them -inf or NaN: the lowest index)
        if (!(m > -INFINITY)) at = wave_first_max(count, lane, m, [&](int n) { return weight_or_least(logw(n)); });
        return at;
    }
    if (POSTERIOR) {
        float m = -INFINITY;
        for (int n = lane; n < count; n += 64) {
            const float v = score(n);
            m = (v > m || v != v) ? v : m;
        }
        m = wave_max_nan(m);
        // (wave-uniform; false for -inf and for NaN: then the bare weights below)
        if (m > -INFINITY) return wave_inverse_cdf(count, lane, u, [&](int n) { return expf(score(n) - m); });
    }
    return wave_inverse_cdf(count, lane, u, [&](int n) { return expf(logw(n)); });
}

template <int MODE, typename ScoreFn, typename LogwFn>
__device__ __forceinline__ int lane_choose(int count, float u, ScoreFn score, LogwFn logw) {
    constexpr bool POSTERIOR = MODE == DPG_MODE_POSTERIOR;
    if (MODE == DPG_MODE_MPE) {
        float m;
        int at = lane_first_max(count, m, score);
        if (!(m > -INFINITY)) at = lane_first_max(count, m, [&](int n) { return weight_or_least(logw(n)); });
        return at;
    }
    if (POSTERIOR) {
        float m = -INFINITY;
        for (int n = 0; n < count; ++n) {
            const float v = score(n);
            m = (v > m || v != v) ? v : m;         // (once NaN, m stays NaN)
        }
        if (m > -INFINITY) return lane_inverse_cdf(count, u, [&](int n) { return expf(score(n) - m); });
    }
    return lane_inverse_cdf(count, u, [&](int n) { return expf(logw(n)); });
}

// MODE: DPG_MODE_PRIOR (act is not read), DPG_MODE_POSTERIOR or DPG_MODE_MPE (the scores of mode 2, selected from)
template <int MODE>
__global__ __launch_bounds__(kThreads) void dgcspn_topdown_kernel(const TopDownArgs a) {
    constexpr bool POSTERIOR = MODE != DPG_MODE_PRIOR;
    extern __shared__ int td_lists[];               // [2][cap]
    __shared__ int td_count[DPG_MAX_LEVELS];        // entries of the list of map j (the input map of product level j)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = a.H * a.W, CHW = a.C * HW, L = a.L, cap = a.cap;
    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const unsigned long long ctr0 = (unsigned long long)b * a.slots;
        float *out = a.out + b * CHW;
        const float *x = a.x ? a.x + b * CHW : nullptr;
        int *choice = a.choice ? a.choice + b * (int64_t)(1 + HW) : nullptr;
        // ---- every pixel as given (out of scope until a path reaches it), every list empty ----
        for (int i = tid; i < CHW; i += kThreads) out[i] = x ? x[i] : NAN;
        if (choice != nullptr)
            for (int i = tid; i < HW; i += kThreads) choice[1 + i] = -1;
        if (tid < L) td_count[tid] = 0;
        int *cur = td_lists, *nxt = td_lists + cap;
        __syncthreads();
        // ---- root: one of the Cr Hr Wr products of the last level, by wave 0 ----
        if (wave == 0) {
            const Level &g = a.lv[L - 1];
            const int hw = g.hout * g.wout, count = g.cout * hw;
            // (a label outside [0, classes) is clamped: a kernel cannot raise, and must not read past the table)
            const int cls = a.y ? min(max((int)a.y[b], 0), a.classes - 1) : 0;
            const float *A = POSTERIOR ? a.act[L - 1] + b * ((int64_t)g.cin * g.hin * g.win) : nullptr;
            const float *lw = a.logw[L] + (int64_t)cls * count;
            const int n = wave_choose<MODE>(
                count, lane, draw_uniform<MODE>(a.seed, ctr0),
                [&](int q) {
                    const int oc = q / hw, p = q - oc * hw, oh = p / g.wout;
                    return prod_value(g, A, oc, oh, p - oh * g.wout) + lw[q];
                },
                [&](int q) { return lw[q]; });
            if (lane == 0) {
                if (choice != nullptr) choice[0] = n;
                const int oc = n / hw, p = n - oc * hw, oh = p / g.wout;
                activate(g, oc, oh, p - oh * g.wout, cur, &td_count[L - 1], cap);
            }
        }
        __syncthreads();
        // ---- sum layers, top to bottom: layer t sits on product level t - 1, its active positions are list t ----
        for (int t = L - 1; t >= 1; --t) {
            const Level &g = a.lv[t - 1];
            const int hw = g.hout * g.wout, count = g.cout;
            const int ncur = min(td_count[t], cap);
            const float *A = POSTERIOR ? a.act[t - 1] + b * ((int64_t)g.cin * g.hin * g.win) : nullptr;
            const unsigned long long ctr = ctr0 + a.base[t];
            if (count > kWide) {
                for (int e = wave; e < ncur; e += kWaves) {
                    const int pk = cur[e], p = pk & 0xffff, oh = p / g.wout, ow = p - oh * g.wout;
                    const float *lw = a.logw[t] + (int64_t)(pk >> 16) * count * hw + p;
                    const int c = wave_choose<MODE>(
                        count, lane, draw_uniform<MODE>(a.seed, ctr + (unsigned)p),
                        [&](int n) { return prod_value(g, A, n, oh, ow) + lw[(int64_t)n * hw]; },
                        [&](int n) { return lw[(int64_t)n * hw]; });
                    if (lane == 0) activate(g, c, oh, ow, nxt, &td_count[t - 1], cap);
                }
            } else {
                for (int e = tid; e < ncur; e += kThreads) {
                    const int pk = cur[e], p = pk & 0xffff, oh = p / g.wout, ow = p - oh * g.wout;
                    const float *lw = a.logw[t] + (int64_t)(pk >> 16) * count * hw + p;
                    const int c = lane_choose<MODE>(
                        count, draw_uniform<MODE>(a.seed, ctr + (unsigned)p),
                        [&](int n) { return prod_value(g, A, n, oh, ow) + lw[(int64_t)n * hw]; },
                        [&](int n) { return lw[(int64_t)n * hw]; });
                    activate(g, c, oh, ow, nxt, &td_count[t - 1], cap);
                }
            }
            __syncthreads();
            int *sw = cur;
            cur = nxt;
            nxt = sw;
        }
        // ---- leaves: every reached pixel from its component, channel by channel ----
        const int n0 = min(td_count[0], cap);
        for (int e = tid; e < n0; e += kThreads) {
            const int pk = cur[e], p = pk & 0xffff, k = pk >> 16;
            if (choice != nullptr) choice[1 + p] = k;
            for (int c = 0; c < a.C; ++c) {
                const int f = c * HW + p;
                const float xv = x ? x[f] : NAN;
                if (xv != xv) {
                    const int64_t po = (int64_t)k * CHW + f;
                    if (MODE == DPG_MODE_MPE) {
                        out[f] = a.loc[po];
                        continue;
                    }
                    const unsigned long long slot = ctr0 + a.base[L] + 2ull * (unsigned long long)f;
                    const float u1 = dp_device::counter_uniform(a.seed, slot), u2 = dp_device::counter_uniform(a.seed, slot + 1ull);
                    const float z = sqrtf(-2.f * logf(1.f - u1)) * cosf(6.28318530717958647692f * u2);
                    out[f] = fmaf(a.scale[po], z, a.loc[po]);
                }
            }
        }
        // (the lists and their counters are rewritten only after every thread has passed the reads above)
        __syncthreads();
    }
}

}  // namespace dpg_detail

using namespace dpg_detail;

extern "C" const char *dpg_last_error(void) { return g_error; }

extern "C" int dpg_abi_version(void) { return 1; }

extern "C" int dpg_dgcspn_topdown(int32_t mode, int64_t B, int32_t C, int32_t H, int32_t W, int32_t K, int32_t n_levels,
                                  const int32_t *geom, int32_t classes, const float *x, const int64_t *y,
                                  const float *const *act, const float *const *logw, const float *loc, const float *scale,
                                  uint64_t seed, float *out, int32_t *choice, void *stream) {
    DPG_REQUIRE(mode == DPG_MODE_PRIOR || mode == DPG_MODE_POSTERIOR || mode == DPG_MODE_MPE, "dpg_dgcspn_topdown: mode %d", mode);
    DPG_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && K > 0 && classes > 0, "dpg_dgcspn_topdown: bad sizes");
    DPG_REQUIRE(logw != nullptr, "dpg_dgcspn_topdown: null table");
    DPG_REQUIRE((int64_t)C * H * W <= (1 << 28), "dpg_dgcspn_topdown: an image of more than 2^28 entries");
    TopDownArgs a{};
    a.B = B; a.C = C; a.H = H; a.W = W; a.K = K; a.L = n_levels; a.classes = classes;
    a.x = mode != DPG_MODE_PRIOR ? x : nullptr;
    a.y = y; a.loc = loc; a.scale = scale; a.seed = seed; a.out = out; a.choice = choice;
    if (int rc = parse_geometry("dpg_dgcspn_topdown", n_levels, geom, K, H, W, a.lv)) return rc;
    int64_t cap = 4, slots = 1;
    for (int j = 0; j < n_levels; ++j) {
        const Level &g = a.lv[j];
        // entries of list j: at most the positions of the map, at most 4 per active node above
        const int64_t above = std::min<int64_t>((int64_t)1 << (2 * std::min(n_levels - j, 8)), 65536);
        cap = std::max<int64_t>(cap, std::min<int64_t>((int64_t)g.hin * g.win, above));
        if (j + 1 < n_levels) {
            a.base[j + 1] = (unsigned)slots;
            slots += (int64_t)g.hout * g.wout;
        }
    }
    a.base[n_levels] = (unsigned)slots;
    a.slots = (unsigned long long)(slots + 2 * (int64_t)C * H * W);
    // (two lists of `cap` ints: 32 KiB at the most, inside the 64 KiB a launch gets without asking for more)
    DPG_REQUIRE(cap <= 4096, "dpg_dgcspn_topdown: %lld active positions at one level are more than the 4096 the lists hold",
                (long long)cap);
    a.cap = (int)cap;
    if (B == 0) return DPG_OK;
    DPG_REQUIRE(loc && scale && out, "dpg_dgcspn_topdown: null pointer");
    DPG_REQUIRE(mode == DPG_MODE_PRIOR || act, "dpg_dgcspn_topdown: modes 2 and 3 need the bottom-up activations");
    for (int t = 0; t < n_levels; ++t) {
        a.act[t] = mode != DPG_MODE_PRIOR ? act[t] : nullptr;
        DPG_REQUIRE(mode == DPG_MODE_PRIOR || a.act[t], "dpg_dgcspn_topdown: activations of level %d missing", t);
    }
    for (int t = 1; t <= n_levels; ++t) {
        a.logw[t] = logw[t];
        DPG_REQUIRE(a.logw[t], "dpg_dgcspn_topdown: log-weights of level %d missing", t);
    }
    const size_t lds = (size_t)2 * a.cap * sizeof(int);
    const unsigned grid = (unsigned)std::min<int64_t>(B, (int64_t)device_cus() * 8);
    if (mode == DPG_MODE_MPE)
        DPG_LAUNCH("dgcspn_topdown_kernel<mpe>", dgcspn_topdown_kernel<DPG_MODE_MPE>, dim3(grid), dim3(kThreads), lds,
                   (hipStream_t)stream, a);
    else if (mode == DPG_MODE_POSTERIOR)
        DPG_LAUNCH("dgcspn_topdown_kernel<posterior>", dgcspn_topdown_kernel<DPG_MODE_POSTERIOR>, dim3(grid), dim3(kThreads), lds,
                   (hipStream_t)stream, a);
    else
        DPG_LAUNCH("dgcspn_topdown_kernel<prior>", dgcspn_topdown_kernel<DPG_MODE_PRIOR>, dim3(grid), dim3(kThreads), lds,
                   (hipStream_t)stream, a);
    return DPG_OK;
}
