// Exact posterior moments of the unobserved variables of a RAT-SPN in ONE launch: RatSpn.posterior_moments, .expectation
// and .variance.  The reference has no counterpart for its tensorized models (deeprob/spn/models/ratspn.py offers mpe and
// sample only); the node-graph path's deeprob.spn.algorithms.moments computes the same quantity on a node graph.
//
// Definition (tests/ratspn_moments_ref.py restates it in numpy, float64 where this file has fp32).  For a row b, from the
// activations act[t] of the bottom-up pass under the evidence (RatSpn._upward_for_mpe):
//   root:    s(q) = fl(fl(a_i + a_j) + lw(q)) over the reps N^2 inputs of the row's class -- the scores of modes 0 / 2 of
//            dpk_ratspn_topdown, fp32, the same operand order; over all C reps N^2 inputs of all classes when no label is
//            given and all_classes is set (the posterior mixture over classes under the uniform class prior);
//            m = max_q s(q), e(q) = expf(s(q) - m), r(q) = e(q) / sum e;
//            F[2p][i] = sum_j r(p, i, j), F[2p + 1][j] = sum_i r(p, i, j);
//   level t, top to bottom: for region g and node o with F[g][o] > 0 the scores of that node's N^2 inputs with the weights
//            logw[t][g, o, :], m / e / r as above (normalised by the node's own sum, not by the stored activation), and
//            F'[2g][i] += F[g][o] sum_j r(i, j), F'[2g + 1][j] += F[g][o] sum_i r(i, j);
//   leaves:  for a NaN variable f, over every repetition and channel k of its leaf region (through `src`):
//            w = sum F_k, mean = sum F_k m_k / w, var = sum F_k (v_k + (m_k - mean)^2) / w
//            with (m_k, v_k) = (loc, scale^2) or (p, p (1 - p)), p = sigmoid(logit);
//   an observed entry returns x[b, f] bit for bit and var 0; a row whose root maximum is -inf or NaN returns NaN in its NaN
//   entries.
//
// Organisation.  A work-group of 256 threads owns a row (grid-stride over rows): the wide model has 2 048 root scores and
// 65 536 level-1 scores a row, a wave alone would walk them in ~1 100 steps a lane and a batch of a few hundred rows would
// fill a fraction of the chip; four waves a row quarter the latency of a row and still leave 5 rows resident a compute unit.
// The subtrees of the repetitions are independent below the root, so the row is walked one repetition at a time and the flow
// tables in LDS are those of ONE repetition: level t's table has 2^(depth - t) regions x N_t nodes, two tables ping-pong by
// the parity of t (~1.5 x 2^depth x max(I, S) floats whatever reps is).
//   * root: three passes of the whole work-group over the scores (maximum, sum of e, then per repetition the N^2 cells
//     e / sum -- added over the classes -- whose row and column sums are the flows into the repetition's two top regions);
//   * a sum level: a wave per region (two waves a region, each half of the nodes o, at the level with two regions).  A lane
//     holds 4 of the region's N^2 <= 256 cells in registers: fl(a_i + a_j) is formed once, and for every node o with flow the
//     wave forms the scores, their maximum and the sum of e by shuffles and adds F[g][o] e / sum to the cell's register.  The
//     cells go to LDS once per region, and 2 N threads sum its rows and columns into the table below -- no scatter per o;
//   * leaves: a thread per variable.  The repetition's contribution (w_r, mean_r, M2_r = sum F_k (v_k + (m_k - mean_r)^2)) is
//     merged into the running (W, mean, M2) of the variable in LDS by the pairwise update of Chan et al. (delta = mean_r -
//     mean; mean += delta w_r / (W + w_r); M2 += M2_r + delta^2 W w_r / (W + w_r)): the stable form of the definition, one
//     repetition at a time.  Every mean is held as its distance from the variable's first channel (m_k - ref is exact for
//     channels that lie close together), so that the rounding of the variance scales with the spread of the channels and
//     not with |loc|; ref is added once, at the end.  The table of the repetition is also what leaf_flow receives.
// Every sum has a fixed order that depends on the shape only: the same row gives the same bits in any batch and grid.
#include "rat_common.h"
#include "../shared/device.h"
#include <algorithm>

namespace dpr_detail {

using dp_device::block_max_nan;
using dp_device::block_sum;
using dp_device::wave_max_nan;
using dp_device::wave_sum;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCells = DPR_MAX_NODES * DPR_MAX_NODES;   // cells of a region, at most
constexpr int kCellsPerLane = kCells / 64;
constexpr int kRedFloats = 16;

struct MomentsArgs {
    int dist;
    int64_t B;
    int D, depth, reps, I, S, C, d;
    int n_cls;                              // classes the root ranges over when y is null: 1 (class 0) or C
    const float *x;                         // [B, D]
    const int64_t *y;                       // [B] or null
    const float *act[DPR_MAX_DEPTH];
    const float *logw[DPR_MAX_DEPTH + 1];
    const int *src;                         // [reps, D]
    const float *p0, *p1;                   // [reps 2^depth, I, d]
    float *mean, *var, *leaf_flow;          // [B, D], [B, D] or null, [B, reps 2^depth, I] or null
    int even_floats, odd_floats;            // sizes of the two flow tables
};

__global__ __launch_bounds__(kThreads) void ratspn_moments_kernel(const MomentsArgs a) {
    extern __shared__ float mo_lds[];
    float *tab_even = mo_lds;                                   // tables of the levels t = 0, 2, ...
    float *tab_odd = tab_even + a.even_floats;                  // t = 1, 3, ...
    float *stat = tab_odd + a.odd_floats;                       // [3][D]: W, mean, M2 of every variable
    float *cells = stat + 3 * (size_t)a.D;                      // [kWaves][kCells]
    float *red = cells + kWaves * kCells;                       // [kRedFloats]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G0 = 1 << a.depth;                                // leaf regions per repetition
    const int D = a.D;
    const int t_top = a.depth - 1;                              // the level the root consumes
    const int Nt = t_top == 0 ? a.I : a.S, NNt = Nt * Nt, RNN = a.reps * NNt;
    const int64_t flow_row = (int64_t)a.reps * G0 * a.I;
    auto leaf_mean = [&](int64_t po) {
        const float q0 = a.p0[po];
        return a.dist == DPR_DIST_GAUSSIAN ? q0 : 1.f / (1.f + expf(-q0));
    };
    // the point the means of variable f are measured from: its first channel in repetition 0
    auto leaf_ref = [&](int f) {
        const int sp = min(max(a.src[f], 0), G0 * a.d - 1), rl = sp / a.d;
        return leaf_mean(((int64_t)rl * a.I) * a.d + (sp - rl * a.d));
    };

    for (int64_t b = blockIdx.x; b < a.B; b += gridDim.x) {
        const float *xrow = a.x + b * D;
        float *mrow = a.mean + b * D;
        float *vrow = a.var ? a.var + b * D : nullptr;
        // (a label outside [0, C) is clamped, as in dpk_ratspn_topdown: a kernel cannot raise and must not read past the table)
        const int cls0 = a.y ? min(max((int)a.y[b], 0), a.C - 1) : 0;
        const int ncls = a.y ? 1 : a.n_cls;
        const float *A = a.act[t_top] + b * (int64_t)(2 * a.reps) * Nt;
        const float *lw = a.logw[a.depth] + (int64_t)cls0 * RNN;
        const int Q = ncls * RNN;
        auto score = [&](int q) {
            const int c = q / RNN, rem = q - c * RNN;
            const int p = rem / NNt, e = rem - p * NNt, i = e / Nt, j = e - i * Nt;
            return (A[(2 * p) * Nt + i] + A[(2 * p + 1) * Nt + j]) + lw[q];
        };
        // ---- root: maximum and normaliser over all of its inputs ----
        float m = -INFINITY;
        for (int q = tid; q < Q; q += kThreads) {
            const float v = score(q);
            m = (v > m || v != v) ? v : m;
        }
        m = block_max_nan<kWaves>(m, red);
        if (!(m > -INFINITY)) {
            // evidence impossible under the model (or undefined): NaN in the NaN entries, the observed ones as given
            for (int f = tid; f < D; f += kThreads) {
                const float xv = xrow[f];
                mrow[f] = xv;
                if (vrow) vrow[f] = xv != xv ? NAN : 0.f;
            }
            if (a.leaf_flow)
                for (int64_t q = tid; q < flow_row; q += kThreads) a.leaf_flow[b * flow_row + q] = NAN;
            continue;                                           // (uniform over the work-group)
        }
        float tot = 0.f;
        for (int q = tid; q < Q; q += kThreads) tot += expf(score(q) - m);
        tot = block_sum<kWaves>(tot, red);
        for (int f = tid; f < D; f += kThreads) {               // (a variable belongs to one thread throughout)
            stat[f] = 0.f;
            stat[D + f] = 0.f;
            stat[2 * D + f] = 0.f;
        }

        for (int rep = 0; rep < a.reps; ++rep) {
            // ---- root: the flows into the two top regions of this repetition ----
            {
                float *T = (t_top & 1) ? tab_odd : tab_even;
                if (tid < NNt) {
                    float c = 0.f;
                    for (int cc = 0; cc < ncls; ++cc) c += expf(score(cc * RNN + rep * NNt + tid) - m);
                    cells[tid] = c / tot;
                }
                __syncthreads();
                if (tid < 2 * Nt) {
                    const int side = tid / Nt, n = tid - side * Nt;
                    float s = 0.f;
                    for (int k = 0; k < Nt; ++k) s += side == 0 ? cells[n * Nt + k] : cells[k * Nt + n];
                    T[side * Nt + n] = s;
                }
                __syncthreads();
            }
            // ---- sum levels, top to bottom: level t has G = 2^(depth - t) regions in the repetition ----
            for (int t = t_top; t >= 1; --t) {
                const int G = 1 << (a.depth - t);
                const int N = t == 1 ? a.I : a.S, NN = N * N;   // nodes of the level below = inputs per child region
                const float *parent = (t & 1) ? tab_odd : tab_even;
                float *child = (t & 1) ? tab_even : tab_odd;
                const float *Ac = a.act[t - 1] + b * (int64_t)(2 * G * a.reps) * N;
                const int P = G == 2 ? 2 : 1;                   // waves per region (G is 2 or a multiple of kWaves)
                const int RP = kWaves / P;                      // regions per step of the work-group
                const int per = (a.S + P - 1) / P;
                for (int gl0 = 0; gl0 < G; gl0 += RP) {
                    const int gl = gl0 + wave / P, part = wave % P;
                    const int g = rep * G + gl;
                    const int o0 = part * per, o1 = min(a.S, o0 + per);
                    float aij[kCellsPerLane], acc[kCellsPerLane];
#pragma unroll
                    for (int c = 0; c < kCellsPerLane; ++c) {
                        const int q = lane + 64 * c;
                        acc[c] = 0.f;
                        aij[c] = 0.f;
                        if (q < NN) {
                            const int i = q / N, j = q - i * N;
                            aij[c] = Ac[(2 * g) * N + i] + Ac[(2 * g + 1) * N + j];
                        }
                    }
                    for (int o = o0; o < o1; ++o) {
                        const float Fo = parent[gl * a.S + o];
                        if (!(Fo > 0.f)) continue;              // (uniform over the wave)
                        const float *lwp = a.logw[t] + ((int64_t)g * a.S + o) * NN;
                        float s[kCellsPerLane];
                        float mo = -INFINITY;
#pragma unroll
                        for (int c = 0; c < kCellsPerLane; ++c) {
                            const int q = lane + 64 * c;
                            s[c] = -INFINITY;
                            if (q < NN) {
                                s[c] = aij[c] + lwp[q];
                                mo = (s[c] > mo || s[c] != s[c]) ? s[c] : mo;
                            }
                        }
                        mo = wave_max_nan(mo);
                        float es = 0.f;
#pragma unroll
                        for (int c = 0; c < kCellsPerLane; ++c) {
                            s[c] = (lane + 64 * c < NN) ? expf(s[c] - mo) : 0.f;
                            es += s[c];
                        }
                        const float scale = Fo / wave_sum(es);
#pragma unroll
                        for (int c = 0; c < kCellsPerLane; ++c) acc[c] += s[c] * scale;
                    }
#pragma unroll
                    for (int c = 0; c < kCellsPerLane; ++c) {
                        const int q = lane + 64 * c;
                        if (q < NN) cells[wave * kCells + q] = acc[c];
                    }
                    __syncthreads();
                    if (tid < RP * 2 * N) {
                        const int r = tid / (2 * N), u = tid - r * 2 * N, side = u / N, n = u - side * N;
                        float sum = 0.f;
                        for (int pp = 0; pp < P; ++pp) {
                            const float *cw = cells + (r * P + pp) * kCells;
                            for (int k = 0; k < N; ++k) sum += side == 0 ? cw[n * N + k] : cw[k * N + n];
                        }
                        child[(2 * (gl0 + r) + side) * N + n] = sum;
                    }
                    __syncthreads();
                }
            }
            // ---- leaves of this repetition ----
            const float *T0 = tab_even;                         // [G0, I]
            if (a.leaf_flow) {
                float *lf = a.leaf_flow + b * flow_row + (int64_t)rep * G0 * a.I;
                for (int q = tid; q < G0 * a.I; q += kThreads) lf[q] = T0[q];
            }
            const int *src = a.src + (int64_t)rep * D;
            for (int f = tid; f < D; f += kThreads) {
                const float xv = xrow[f];
                if (xv == xv) continue;
                const int sp = src[f], rl = sp / a.d, j = sp - rl * a.d;
                if (sp < 0 || rl >= G0) continue;               // (never with the tables of RatSpn._topdown_src)
                const int64_t po = ((int64_t)(rep * G0 + rl) * a.I) * a.d + j;
                const float *Fk = T0 + rl * a.I;
                const float ref = leaf_ref(f);
                float w = 0.f, sm = 0.f;
                for (int k = 0; k < a.I; ++k) {
                    w += Fk[k];
                    sm += Fk[k] * (leaf_mean(po + (int64_t)k * a.d) - ref);
                }
                if (!(w > 0.f)) continue;                       // (this repetition has no share of the posterior)
                const float mr = sm / w;
                float M2r = 0.f;
                for (int k = 0; k < a.I; ++k) {
                    const float mk = leaf_mean(po + (int64_t)k * a.d);
                    float vk;
                    if (a.dist == DPR_DIST_GAUSSIAN) {
                        const float sc = a.p1[po + (int64_t)k * a.d];
                        vk = sc * sc;
                    } else {
                        vk = mk * (1.f - mk);
                    }
                    const float dl = (mk - ref) - mr;
                    M2r += Fk[k] * (vk + dl * dl);
                }
                const float W = stat[f], mu = stat[D + f], M2 = stat[2 * D + f];
                const float Wn = W + w, frac = w / Wn, delta = mr - mu;
                stat[f] = Wn;
                stat[D + f] = mu + delta * frac;
                stat[2 * D + f] = M2 + M2r + delta * delta * (W * frac);
            }
            __syncthreads();                                    // (the tables are rewritten by the next repetition)
        }
        for (int f = tid; f < D; f += kThreads) {
            const float xv = xrow[f];
            float mean = xv, var = 0.f;
            if (xv != xv) {
                const float W = stat[f];
                mean = W > 0.f ? leaf_ref(f) + stat[D + f] : NAN;
                var = stat[2 * D + f] / W;
            }
            mrow[f] = mean;
            if (vrow) vrow[f] = var;
        }
    }
}

}  // namespace dpr_detail

using namespace dpr_detail;

extern "C" const char *dpr_last_error(void) { return g_error; }

extern "C" int dpr_abi_version(void) { return 1; }

extern "C" int dpr_ratspn_moments(int32_t dist, int64_t B, int32_t D, int32_t depth, int32_t reps, int32_t I, int32_t S,
                                  int32_t C, int32_t d, const float *x, const int64_t *y, int32_t all_classes,
                                  const float *const *act, const float *const *logw, const int32_t *src,
                                  const float *p0, const float *p1, float *mean, float *var, float *leaf_flow,
                                  void *stream) {
    DPR_REQUIRE(dist == DPR_DIST_GAUSSIAN || dist == DPR_DIST_BERNOULLI, DPR_EINVAL, "ratspn_moments: dist %d", dist);
    DPR_REQUIRE(B >= 0 && D > 0 && depth >= 1 && reps > 0 && I > 0 && S > 0 && C > 0 && d > 0, DPR_EINVAL,
                "ratspn_moments: bad sizes (B %lld, D %d, depth %d, reps %d, I %d, S %d, C %d, d %d)", (long long)B, D, depth,
                reps, I, S, C, d);
    DPR_REQUIRE(depth <= DPR_MAX_DEPTH && I <= DPR_MAX_NODES && S <= DPR_MAX_NODES, DPR_EUNSUPPORTED,
                "ratspn_moments: depth %d, I %d, S %d outside the envelope (depth <= %d, I and S <= %d)", depth, I, S,
                DPR_MAX_DEPTH, DPR_MAX_NODES);
    const int64_t N = depth == 1 ? I : S;
    DPR_REQUIRE((int64_t)C * reps * N * N <= (1 << 30) && (int64_t)reps * ((int64_t)1 << depth) * I * (int64_t)d <= (1ll << 31) - 1
                    && (int64_t)reps * D <= (1ll << 31) - 1,
                DPR_EUNSUPPORTED, "ratspn_moments: C %d x reps %d x N^2 %lld root inputs or reps x 2^depth x I x d leaf "
                "parameters beyond 32-bit indices", C, reps, (long long)(N * N));
    int64_t even = 0, odd = 0;
    for (int t = 0; t < depth; ++t) {
        const int64_t sz = ((int64_t)1 << (depth - t)) * (t == 0 ? I : S);
        if (t & 1) odd = std::max(odd, sz); else even = std::max(even, sz);
    }
    const int64_t lds = 4 * (even + odd + 3 * (int64_t)D + kWaves * kCells + kRedFloats);
    DPR_REQUIRE(lds <= DPR_MAX_LDS_BYTES, DPR_EUNSUPPORTED,
                "ratspn_moments: the tables of a row need %lld bytes of LDS (flow tables %lld + %lld floats, 3 x %d moment "
                "accumulators), the limit is %d", (long long)lds, (long long)even, (long long)odd, D, DPR_MAX_LDS_BYTES);
    if (B == 0) return DPR_OK;
    DPR_REQUIRE(x && act && logw && src && p0 && mean && (dist == DPR_DIST_BERNOULLI || p1), DPR_EINVAL,
                "ratspn_moments: null pointer");
    MomentsArgs a{};
    a.dist = dist; a.B = B; a.D = D; a.depth = depth; a.reps = reps; a.I = I; a.S = S; a.C = C; a.d = d;
    a.n_cls = (y == nullptr && all_classes) ? C : 1;
    a.x = x; a.y = y; a.src = src; a.p0 = p0; a.p1 = p1; a.mean = mean; a.var = var; a.leaf_flow = leaf_flow;
    a.even_floats = (int)even; a.odd_floats = (int)odd;
    for (int t = 0; t < depth; ++t) {
        a.act[t] = act[t];
        DPR_REQUIRE(a.act[t], DPR_EINVAL, "ratspn_moments: activations of level %d missing", t);
    }
    for (int t = 1; t <= depth; ++t) {
        a.logw[t] = logw[t];
        DPR_REQUIRE(a.logw[t], DPR_EINVAL, "ratspn_moments: log-weights of level %d missing", t);
    }
    if (lds > 65536) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ratspn_moments_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        DPR_REQUIRE(e == hipSuccess, DPR_ELAUNCH, "hipFuncSetAttribute(max dynamic LDS = %lld): %s", (long long)lds,
                    hipGetErrorString(e));
    }
    const unsigned grid = (unsigned)std::min<int64_t>(B, (int64_t)device_cus() * 8);
    DPR_LAUNCH("ratspn_moments_kernel", ratspn_moments_kernel, dim3(grid), dim3(kThreads), (size_t)lds, (hipStream_t)stream, a);
    return DPR_OK;
}
