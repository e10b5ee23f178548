// Exact posterior moments of the missing entries of a DGC-SPN in ONE launch: DgcSpn.posterior_moments, .expectation and
// .variance (include/deeprob_dgcm.h).
//
// reference: deeprob/spn/models/dgcspn.py offers `mpe` only -- autograd through every layer, every product map written, the
// flow of a sum node normalised by the stored fp32 activation, means without variances.  csrc/rat/ratspn_moments.hip is the
// same pass for RAT-SPNs.
//
// Definition (tests/dgcspn_moments_ref.py restates it in numpy, float64 where this file has fp32).  Inputs are those of
// dpg_dgcspn_topdown in mode 2 (csrc/dgc/dgcspn_topdown.hip): x, y, act[0 .. L-1], logw[1 .. L], geom, loc, scale.  Product
// values, tap coordinates and the channel decode are those of include/deeprob_dgc.h: a product is ((v0 + v1) + v2) + v3 in
// fp32, a tap outside the map is 0 and receives nothing.  P_j is the (never stored) product map of level j, G_j the flow
// into it, F_j the flow into the map level j reads (F_0: the leaf map, F_t: the map of sum layer t).  Per image:
//   1. Root.  s(i) = P_{L-1}(i) + logw[L][cls, i] over the flattened last product map, m = max s, e = expf(s - m),
//      G_{L-1}(i) = e(i) / sum e.  Without labels and with all_classes, s ranges over all classes x N entries at once and
//      G(i) is the sum over the classes (the mixture of the classes under the uniform class prior).  m = -inf or NaN: the
//      evidence is impossible, the image's NaN entries are NaN in mean and var, leaf_flow is NaN.
//   2. Product level j = L-1 .. 0.  Every product (oc, oh, ow) passes its flow to each of its taps inside the map:
//      F_j[c_t, ih, iw] += G_j[oc, oh, ow].  Computed as a gather, so that the sum has a fixed order: an input position is
//      tapped by at most four output positions, one per tap t = 0 .. 3 in this order, and at a level that is not depthwise
//      by the Cin^3 output channels whose digit t is the input channel, in increasing oc.
//   3. Sum layer t = j (j >= 1).  For every position (h, w) and every output o with F_t[o, h, w] > 0:
//      s(c) = P_{t-1}(c, h, w) + logw[t][o, c, h, w], m = max_c s, e = expf(s - m), r = e / sum_c e -- normalised by the
//      node's own sum, not by the stored activation -- and G_{t-1}[c, h, w] = sum_o F_t[o, h, w] r(o, c), o increasing.
//   4. Leaves.  F_0[k, h, w] is the flow of component k (= d log p / d act[0], what leaf_flow receives), w = sum_k F_0.
//      For a NaN entry (c, h, w) with w > 0, with ref = loc[0, c, h, w] and d_k = loc[k, c, h, w] - ref:
//      mr = sum_k F_0 d_k / w, mean = ref + mr, var = sum_k F_0 (scale_k^2 + (d_k - mr)^2) / w  (never E[x^2] - mean^2: the
//      rounding of the variance scales with the spread of the components, not with |loc|).  w = 0: the pixel is in nobody's
//      scope and stays NaN in both outputs.  An observed entry returns x bit for bit and var 0.
//
// Organisation.  A work-group of 512 threads owns an image, grid-stride over the batch.  The flow maps do not fit in LDS at
// the sizes that matter (the sum maps of the 28 x 28 example model are 32 x 59 x 59 floats = 445 KB), so the work-group owns
// a slice of the caller's workspace with two buffers, F (largest input map) and G (largest product map), written and read
// by this work-group only; F_t overwrites F_{t+1} once G_t is formed; the phases are separated by __syncthreads().  Small
// images take the same route (their slices stay in L2).
//   * root: three passes of the work-group over the scores (maximum, sum of e, the cells), wave then work-group reductions;
//   * a product level: a thread per element of F_j gathers its at most four (times Cin^3) cells of G_j -- every element of
//     F_j is written, nothing is zeroed beforehand and nothing is added atomically;
//   * a sum layer of at most 32 inputs a node: a thread per position (the loads of a wave are contiguous along w).  The
//     node's product values do not depend on the output o, so they are formed once per position and kept in registers with
//     the position's cells of G; per output o one load of logw per input, the maximum, e and its sum, the shares.  The
//     arrays are statically indexed (unrolled loops over CMAX guarded by c < count); the kernel is built for CMAX = 8 and
//     CMAX = 32 and the launch takes the smaller one that holds the model's nodes, so that an 8-channel model does not pay
//     the registers of a 32-channel one;
//   * a wider node (81 product channels, say): a wave per position, the lanes over the inputs, three passes over them per
//     output o (maximum, sum of e, the shares -- recomputed per pass, not kept), maximum and sum by
//     dp_device::wave_max_nan / wave_sum, the shares added to the lane's own cells of G, which it zeroed itself;
//   * leaves: a thread per entry (c, h, w).
// Every sum has an order that depends on the shape only: the same image gives the same bits in any batch and grid.
#include "dgc_common.h"
#include "../../../include/deeprob_dgcm.h"
#include "../shared/device.h"
#include <algorithm>

static_assert(DPM_OK == DPG_OK && DPM_EINVAL == DPG_EINVAL && DPM_ELAUNCH == DPG_ELAUNCH, "one library, one set of codes");

namespace dpg_detail {

using dp_device::block_max_nan;
using dp_device::block_sum;
using dp_device::wave_max_nan;
using dp_device::wave_sum;

constexpr int kMoThreads = 512;
constexpr int kMoWaves = kMoThreads / 64;
constexpr int kMoWide = 32;          // a sum node of more inputs than this is walked by a wave
constexpr int kMoSmall = 8;          // the kernel built for nodes of at most this many inputs keeps fewer registers

struct MomentsArgs {
    int64_t B;
    int C, H, W, K, L, classes;
    int n_cls;                           // classes the root ranges over when y is null: 1 (class 0) or `classes`
    Level lv[DPG_MAX_LEVELS];
    const float *x;
    const int64_t *y;
    const float *act[DPG_MAX_LEVELS];
    const float *logw[DPG_MAX_LEVELS + 1];
    const float *loc, *scale;
    float *mean, *var, *leaf_flow;
    float *ws;
    int64_t nF, nG;                      // floats of the two buffers of a slice
};

// CMAX: the most inputs of a sum node that a thread keeps in registers, kMoSmall or kMoWide
template <int CMAX>
__global__ __launch_bounds__(kMoThreads) void dgcspn_moments_kernel(const MomentsArgs a) {
    __shared__ float red[kMoWaves];
    // The geometry is read from LDS where it is used.  Read from the kernel's arguments, every level's fields are hoisted
    // above the batch loop into scalar registers, more than there are: they would be spilled.
    __shared__ Level lv[DPG_MAX_LEVELS];
    for (int i = threadIdx.x; i < a.L * (int)(sizeof(Level) / sizeof(int)); i += kMoThreads)
        reinterpret_cast<int *>(lv)[i] = reinterpret_cast<const int *>(a.lv)[i];
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = a.H * a.W, CHW = a.C * HW, KHW = a.K * HW, L = a.L;
    float *F = a.ws + (int64_t)blockIdx.x * (a.nF + a.nG);
    float *G = F + a.nF;
    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        // ---- root: the share of every product of the last level ----
        {
            const Level g = lv[L - 1];
            const int hw = g.hout * g.wout, N = g.cout * hw;
            // (a label outside [0, classes) is clamped: a kernel cannot raise, and must not read past the table)
            const int cls0 = a.y ? min(max((int)a.y[b], 0), a.classes - 1) : 0;
            const int ncls = a.y ? 1 : a.n_cls;
            const float *A = a.act[L - 1] + b * ((int64_t)g.cin * g.hin * g.win);
            const float *lw = a.logw[L] + (int64_t)cls0 * N;
            auto score = [&](int cc, int i) {
                const int oc = i / hw, p = i - oc * hw, oh = p / g.wout;
                return prod_value(g, A, oc, oh, p - oh * g.wout) + lw[cc * N + i];
            };
            float m = -INFINITY;
            for (int cc = 0; cc < ncls; ++cc)
                for (int i = tid; i < N; i += kMoThreads) {
                    const float v = score(cc, i);
                    m = (v > m || v != v) ? v : m;
                }
            m = block_max_nan<kMoWaves>(m, red);
            if (!(m > -INFINITY)) {
                // evidence impossible under the model (or undefined): NaN in the NaN entries, the observed ones as given
                for (int f = tid; f < CHW; f += kMoThreads) {
                    const float xv = a.x[b * CHW + f];
                    a.mean[b * CHW + f] = xv;
                    if (a.var) a.var[b * CHW + f] = xv != xv ? NAN : 0.f;
                }
                if (a.leaf_flow)
                    for (int q = tid; q < KHW; q += kMoThreads) a.leaf_flow[b * KHW + q] = NAN;
                continue;                                       // (uniform over the work-group)
            }
            float tot = 0.f;
            for (int cc = 0; cc < ncls; ++cc)
                for (int i = tid; i < N; i += kMoThreads) tot += expf(score(cc, i) - m);
            tot = block_sum<kMoWaves>(tot, red);
            for (int i = tid; i < N; i += kMoThreads) {
                float c = 0.f;
                for (int cc = 0; cc < ncls; ++cc) c += expf(score(cc, i) - m);
                G[i] = c / tot;
            }
            __syncthreads();
        }
        for (int j = L - 1; j >= 0; --j) {
            // ---- product level j: F_j gathers G_j ----
            const Level g = lv[j];
            const int hwin = g.hin * g.win, hwout = g.hout * g.wout, nin = g.cin * hwin;
            for (int idx = tid; idx < nin; idx += kMoThreads) {
                const int c = idx / hwin, p = idx - c * hwin, ih = p / g.win, iw = p - ih * g.win;
                float f = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int nh = ih + g.pt - (t >> 1) * g.dil, nw = iw + g.pl - (t & 1) * g.dil;
                    if (nh < 0 || nw < 0) continue;
                    const int oh = nh / g.stride, ow = nw / g.stride;
                    if (oh * g.stride != nh || ow * g.stride != nw || oh >= g.hout || ow >= g.wout) continue;
                    const int po = oh * g.wout + ow;
                    if (g.dw) {
                        f += G[c * hwout + po];
                    } else {
                        // the output channels whose digit t is c: (hi Cin + c) span + lo, increasing
                        const int span = t == 0 ? g.cin3 : t == 1 ? g.cin2 : t == 2 ? g.cin : 1;
                        const int nhi = g.cout / (span * g.cin);
                        for (int hi = 0; hi < nhi; ++hi)
                            for (int lo = 0; lo < span; ++lo) f += G[((hi * g.cin + c) * span + lo) * hwout + po];
                    }
                }
                F[idx] = f;
            }
            __syncthreads();
            if (j == 0) break;
            // ---- sum layer t = j on product level j - 1: G_{j-1} from F_j ----
            const Level gp = lv[j - 1];
            const int count = gp.cout, hw = hwin;               // (hin_j x win_j = hout_{j-1} x wout_{j-1})
            const float *A = a.act[j - 1] + b * ((int64_t)gp.cin * gp.hin * gp.win);
            const float *lwt = a.logw[j];
            if (count > kMoWide) {
                for (int p = wave; p < hw; p += kMoWaves) {
                    const int oh = p / gp.wout, ow = p - oh * gp.wout;
                    #pragma nounroll
                    for (int c = lane; c < count; c += 64) G[c * hw + p] = 0.f;
                    #pragma nounroll
                    for (int o = 0; o < g.cin; ++o) {
                        const float Fo = F[o * hw + p];
                        if (!(Fo > 0.f)) continue;              // (uniform over the wave)
                        const float *lw = lwt + (int64_t)o * count * hw + p;
                        float m = -INFINITY;
                        #pragma nounroll
                        for (int c = lane; c < count; c += 64) {
                            const float v = prod_value(gp, A, c, oh, ow) + lw[c * hw];
                            m = (v > m || v != v) ? v : m;
                        }
                        m = wave_max_nan(m);
                        float es = 0.f;
                        #pragma nounroll
                        for (int c = lane; c < count; c += 64) es += expf((prod_value(gp, A, c, oh, ow) + lw[c * hw]) - m);
                        const float share = Fo / wave_sum(es);
                        #pragma nounroll
                        for (int c = lane; c < count; c += 64)
                            G[c * hw + p] += expf((prod_value(gp, A, c, oh, ow) + lw[c * hw]) - m) * share;
                    }
                }
            } else {
                // a node's product values do not depend on o: formed once per position and kept, with the shares, in
                // registers (statically indexed: the loops over CMAX are unrolled and guarded by c < count)
                for (int p = tid; p < hw; p += kMoThreads) {
                    const int oh = p / gp.wout, ow = p - oh * gp.wout;
                    float P[CMAX], acc[CMAX];
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        acc[c] = 0.f;
                        P[c] = c < count ? prod_value(gp, A, c, oh, ow) : 0.f;
                    }
#pragma nounroll
                    for (int o = 0; o < g.cin; ++o) {
                        const float Fo = F[o * hw + p];
                        if (!(Fo > 0.f)) continue;
                        const float *lw = lwt + (int64_t)o * count * hw + p;
                        float e[CMAX];
                        float m = -INFINITY;
#pragma unroll
                        for (int c = 0; c < CMAX; ++c)
                            if (c < count) {
                                e[c] = P[c] + lw[c * hw];
                                m = (e[c] > m || e[c] != e[c]) ? e[c] : m;
                            }
                        float es = 0.f;
#pragma unroll
                        for (int c = 0; c < CMAX; ++c)
                            if (c < count) {
                                e[c] = expf(e[c] - m);
                                es += e[c];
                            }
                        const float share = Fo / es;
#pragma unroll
                        for (int c = 0; c < CMAX; ++c)
                            if (c < count) acc[c] += e[c] * share;
                    }
#pragma unroll
                    for (int c = 0; c < CMAX; ++c)
                        if (c < count) G[c * hw + p] = acc[c];
                }
            }
            __syncthreads();
        }
        // ---- leaves: F holds F_0 [K, H, W] ----
        if (a.leaf_flow)
            for (int q = tid; q < KHW; q += kMoThreads) a.leaf_flow[b * KHW + q] = F[q];
        for (int f = tid; f < CHW; f += kMoThreads) {
            const float xv = a.x[b * CHW + f];
            float mu = xv, vr = 0.f;
            if (xv != xv) {
                const int p = f % HW;
                float w = 0.f;
                for (int k = 0; k < a.K; ++k) w += F[k * HW + p];
                vr = NAN;
                if (w > 0.f) {                                  // (else: a pixel in nobody's scope stays NaN)
                    const float ref = a.loc[f];
                    float sm = 0.f;
                    for (int k = 0; k < a.K; ++k) sm += F[k * HW + p] * (a.loc[k * CHW + f] - ref);
                    const float mr = sm / w;
                    float M2 = 0.f;
                    for (int k = 0; k < a.K; ++k) {
                        const float sc = a.scale[k * CHW + f], dl = (a.loc[k * CHW + f] - ref) - mr;
                        M2 += F[k * HW + p] * (sc * sc + dl * dl);
                    }
                    mu = ref + mr;
                    vr = M2 / w;
                }
            }
            a.mean[b * CHW + f] = mu;
            if (a.var) a.var[b * CHW + f] = vr;
        }
        // (the slice is rewritten by the next image only after every thread has passed the reads above)
        __syncthreads();
    }
}

// |F| and |G| of a slice, in floats
static void slice_floats(const Level *lv, int n_levels, int64_t *nF, int64_t *nG) {
    *nF = *nG = 0;
    for (int j = 0; j < n_levels; ++j) {
        *nF = std::max(*nF, (int64_t)lv[j].cin * lv[j].hin * lv[j].win);
        *nG = std::max(*nG, (int64_t)lv[j].cout * lv[j].hout * lv[j].wout);
    }
}

}  // namespace dpg_detail

using namespace dpg_detail;

extern "C" const char *dpm_last_error(void) { return g_error; }

extern "C" int64_t dpm_dgcspn_moments_workspace_bytes(int64_t B, int32_t n_levels, const int32_t *geom) {
    DPG_REQUIRE(B >= 0, "dpm_dgcspn_moments_workspace_bytes: bad sizes (B %lld)", (long long)B);
    Level lv[DPG_MAX_LEVELS];
    if (int rc = parse_geometry("dpm_dgcspn_moments_workspace_bytes", n_levels, geom, 0, 0, 0, lv)) return rc;
    int64_t nF, nG;
    slice_floats(lv, n_levels, &nF, &nG);
    return std::min<int64_t>(B, DPM_MAX_GROUPS) * (nF + nG) * (int64_t)sizeof(float);
}

extern "C" int dpm_dgcspn_moments(int64_t B, int32_t C, int32_t H, int32_t W, int32_t K, int32_t n_levels, const int32_t *geom,
                                  int32_t classes, int32_t all_classes, const float *x, const int64_t *y,
                                  const float *const *act, const float *const *logw, const float *loc, const float *scale,
                                  float *mean, float *var, float *leaf_flow, void *workspace, int64_t workspace_bytes,
                                  void *stream) {
    DPG_REQUIRE(B >= 0 && C > 0 && H > 0 && W > 0 && K > 0 && classes > 0,
                "dpm_dgcspn_moments: bad sizes (B %lld, C %d, H %d, W %d, K %d, classes %d)", (long long)B, C, H, W, K, classes);
    DPG_REQUIRE(logw != nullptr && act != nullptr, "dpm_dgcspn_moments: null table");
    DPG_REQUIRE((int64_t)C * H * W <= (1 << 28) && (int64_t)K * H * W <= 0x7fffffff && (int64_t)K * C * H * W <= 0x7fffffff,
                "dpm_dgcspn_moments: an image of more than 2^28 entries or leaf tables of more than 2^31");
    MomentsArgs a{};
    if (int rc = parse_geometry("dpm_dgcspn_moments", n_levels, geom, K, H, W, a.lv)) return rc;
    const Level &top = a.lv[n_levels - 1];
    DPG_REQUIRE((int64_t)classes * top.cout * top.hout * top.wout <= 0x7fffffff, "dpm_dgcspn_moments: root table too large");
    a.B = B; a.C = C; a.H = H; a.W = W; a.K = K; a.L = n_levels; a.classes = classes;
    a.n_cls = (y == nullptr && all_classes) ? classes : 1;
    a.x = x; a.y = y; a.loc = loc; a.scale = scale; a.mean = mean; a.var = var; a.leaf_flow = leaf_flow;
    slice_floats(a.lv, n_levels, &a.nF, &a.nG);
    if (B == 0) return DPM_OK;
    const int64_t groups = std::min<int64_t>(B, DPM_MAX_GROUPS);
    const int64_t need = groups * (a.nF + a.nG) * (int64_t)sizeof(float);
    DP_REQUIRE(workspace_bytes >= need, DPM_EWORKSPACE, "dpm_dgcspn_moments: the workspace has %lld bytes, %lld work-groups x "
               "(%lld + %lld) floats need %lld", (long long)workspace_bytes, (long long)groups, (long long)a.nF, (long long)a.nG,
               (long long)need);
    DPG_REQUIRE(x && loc && scale && mean && workspace, "dpm_dgcspn_moments: null pointer");
    a.ws = (float *)workspace;
    for (int t = 0; t < n_levels; ++t) {
        a.act[t] = act[t];
        DPG_REQUIRE(a.act[t], "dpm_dgcspn_moments: activations of level %d missing", t);
    }
    for (int t = 1; t <= n_levels; ++t) {
        a.logw[t] = logw[t];
        DPG_REQUIRE(a.logw[t], "dpm_dgcspn_moments: log-weights of level %d missing", t);
    }
    // (the kernel sends a node of more than kMoWide inputs to its waves and every other one to a thread's CMAX registers:
    // CMAX must hold the largest of those, which is what is chosen here)
    int narrow = 0;                      // the most inputs of a sum node among the levels a thread walks alone
    for (int j = 0; j + 1 < n_levels; ++j)
        if (a.lv[j].cout <= kMoWide) narrow = std::max(narrow, a.lv[j].cout);
    if (narrow <= kMoSmall)
        DPG_LAUNCH("dgcspn_moments_kernel<8>", dgcspn_moments_kernel<kMoSmall>, dim3((unsigned)groups), dim3(kMoThreads), 0,
                   (hipStream_t)stream, a);
    else
        DPG_LAUNCH("dgcspn_moments_kernel<32>", dgcspn_moments_kernel<kMoWide>, dim3((unsigned)groups), dim3(kMoThreads), 0,
                   (hipStream_t)stream, a);
    return DPM_OK;
}
