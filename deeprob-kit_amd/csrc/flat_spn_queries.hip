// Queries beyond log_likelihood on a vanilla (node-graph) SPN flattened into arrays: MPE completion, (conditional)
// sampling, per-node log-gradients and the batch EM step.  Same organisation as flat_spn.hip: lane = sample, the node loop
// is uniform over the wave, tables are [row][sample] so that every access is one 256-byte row per wave.
//
// Replaces deeprob/spn/algorithms/evaluation.py:99-177 (eval_top_down) with inference.py:106-126 (mpe) and sampling.py
// (sample; the branch is drawn from the exact posterior, see below), gradient.py:13-63 (eval_backward) and the loop body
// of learning/em.py:84-107 with node.py:100-111 and leaf.py:167-174, 281-293, 536-545 (em_step).
//
// ---- top-down (dpk_flat_spn_topdown) ---------------------------------------------------------------------------------
// One launch: the bottom-up pass of flat_spn.hip, during which every sum node's branch is decided while its children's
// rows are still live in the recycled table (one byte per (sum node, sample)), then the walk from the root over the stored
// order reversed.  Reach flags are one 64-bit lane mask per node (bit = lane = sample); a node whose mask is zero is skipped
// by the whole wave.  LDS route: value rows | reach masks | branch bytes, when they fit in 64 KB; otherwise the same code
// on a caller-supplied workspace (value table with row = node id, branch bytes [n_sum, B], masks [waves, n_nodes]).
//   mpe:    branch = first maximum of ll_child_k + log w_k (float32; log w_k comes from the host, child_logw)
//   sample: with j the mpe branch, t_k = exp((ll_child_k - ll_child_j) + (log w_k - log w_j)), branch = first k with
//           u * sum_i t_i < t_0 + .. + t_k (float32, child order; if rounding leaves none, the last k with t_k > 0): the
//           posterior w_k exp(ll_k) / sum_i w_i exp(ll_i); children that all sit on the -1e31 floor follow the weights
// A reached leaf fills its variable where the input is NaN: mpe -- Bernoulli (p < 0.5 ? 0 : 1), Categorical the category
// of the first largest probability, Uniform start, Gaussian mean; sample -- Bernoulli u1 < p, Categorical inverse CDF over
// the float32 probabilities in category order (same rule as the branch), Uniform start + width u1, Gaussian
// mean + stddev sqrt(-2 log(1 - u1)) cos(2 pi u2).
// Counter layout of the draws (a test replays it): u(ctr) = dp_device::counter_uniform(seed, ctr) (shared/device.h) with
// ctr = b * K + slot, K = n_sum + 2 n_vars; slot s = the branch of the sum node with sum_index s, slots n_sum + 2 v and
// n_sum + 2 v + 1 = u1, u2 of variable v's leaf.
//
// ---- backward (dpk_flat_spn_backward) --------------------------------------------------------------------------------
// grads[root] = 0; parents before children: a sum passes g + log w_k, a product g + ll_node - ll_child; a child's row is
// the running log-add-exp of what its parents pass (all -inf stays -inf).
//
// ---- EM step (dpk_flat_spn_em_step) ----------------------------------------------------------------------------------
// Two launches: (1) forward + backward tables of the batch rows gathered through `index`; (2) one work-group per node
// (+ one for the batch mean of the root) that sums its statistics over the batch in a fixed order in float64 -- every
// thread its strided share, a butterfly over the wave, the waves in order: no atomics, bitwise reproducible -- and applies
// the update to its own parameters (raw and derived).  No work-group reads a parameter another one writes.
#include "common.h"
#include "shared/device.h"
#include "shared/flat_spn_nodes.h"
#include <math.h>

namespace dpk {
namespace fq {

using namespace dp_device::flat;     // the kinds, node_value, log_add_exp
constexpr int kLdsBytes = 65536;
constexpr int kUpdThreads = 256;
using Circuit = dpk_flat_spn_circuit;
typedef unsigned long long u64;
using dp_device::counter_uniform;

__device__ __forceinline__ u64 wave_uniform(u64 v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}

struct TopdownArgs {
    Circuit c;
    float *x;
    int64_t B;
    int D, n_slots;
    u64 seed;
    float *table;            // workspace route: [n_nodes, B]
    unsigned char *branch;   //                  [n_sum, B]
    u64 *reach;              //                  [waves, n_nodes]
};

template <bool kLds, bool kSample>
__global__ __launch_bounds__(64) void flat_topdown_kernel(const TopdownArgs a) {
    extern __shared__ float lds[];
    const Circuit &c = a.c;
    const int lane = threadIdx.x, n = c.n_nodes;
    const int64_t b = (int64_t)blockIdx.x * 64 + lane;
    const bool own = b < a.B;
    const int64_t bb = own ? b : a.B - 1;       // tail lanes shadow the last sample, every store of theirs is masked
    float *xrow = a.x + bb * a.D;
    u64 *reach = kLds ? (u64 *)(lds + a.n_slots * 64) : a.reach + (int64_t)blockIdx.x * n;
    unsigned char *branch = kLds ? (unsigned char *)(reach + n) : a.branch;
    const int32_t *cidx = kLds ? c.child_slot : c.child_index;
    auto load = [&](int row) -> float { return kLds ? lds[row * 64 + lane] : a.table[row * a.B + bb]; };
    const u64 ctr0 = (u64)bb * (u64)(c.n_sum + 2 * c.n_vars);

    // ---- bottom-up, branch of every sum node decided on the way -------------------------------------------------------
    for (int t = 0; t < n; ++t) {
        const int i = c.order[t];
        const int kind = c.kind[i];
        const float v = node_value(c, i, kind, xrow, cidx, load);
        if (kind == kSum) {
            const int c0 = c.arg0[i], nc = c.arg1[i], s = c.sum_index[i];
            float best = -INFINITY, bl = 0.f, bw = 0.f;
            int br = 0;
            for (int j = 0; j < nc; ++j) {
                const float l = load(cidx[c0 + j]), lw = c.child_logw[c0 + j];
                if (j == 0 || l + lw > best) {
                    best = l + lw;
                    bl = l;
                    bw = lw;
                    br = j;
                }
            }
            if (kSample) {
                // the best candidate subtracted in two parts: children that all sit on the floor (where the float32 sum
                // ll + log w has absorbed log w) still follow the weights
                float total = 0.f;
                for (int j = 0; j < nc; ++j) total += expf((load(cidx[c0 + j]) - bl) + (c.child_logw[c0 + j] - bw));
                const float target = counter_uniform(a.seed, ctr0 + (u64)s) * total;
                float cum = 0.f;
                int last = br;
                bool found = false;
                for (int j = 0; j < nc; ++j) {
                    const float tj = expf((load(cidx[c0 + j]) - bl) + (c.child_logw[c0 + j] - bw));
                    cum += tj;
                    if (!found && tj > 0.f) last = j;
                    if (!found && target < cum) {
                        br = j;
                        found = true;
                    }
                }
                if (!found) br = last;
            }
            if (kLds)
                branch[s * 64 + lane] = (unsigned char)br;
            else if (own)
                branch[(int64_t)s * a.B + b] = (unsigned char)br;
        }
        if (kLds)
            lds[c.node_slot[i] * 64 + lane] = v;
        else if (own)
            a.table[(int64_t)i * a.B + b] = v;
    }

    // ---- top-down -----------------------------------------------------------------------------------------------------
    // every lane stores the same mask word, so each lane reads back what it wrote itself
    for (int i = 0; i < n; ++i) reach[i] = 0ull;
    reach[c.root] = __ballot(own);
    for (int t = n - 1; t >= 0; --t) {
        const int i = c.order[t];
        const u64 m = wave_uniform(reach[i]);
        if (m == 0ull) continue;
        const int kind = c.kind[i];
        const bool mine = (m >> lane) & 1ull;
        if (kind == kProduct) {
            const int c0 = c.arg0[i], nc = c.arg1[i];
            for (int j = 0; j < nc; ++j) reach[c.child_index[c0 + j]] |= m;
        } else if (kind == kSum) {
            const int c0 = c.arg0[i], nc = c.arg1[i], s = c.sum_index[i];
            int br = -1;
            if (mine) br = kLds ? branch[s * 64 + lane] : branch[(int64_t)s * a.B + b];
            for (int j = 0; j < nc; ++j) {
                const u64 mj = __ballot(br == j);
                if (mj != 0ull) reach[c.child_index[c0 + j]] |= mj;
            }
        } else if (mine) {
            const int var = c.arg0[i];
            const float xv = xrow[var];
            if (xv != xv) {
                float fill;
                if (!kSample) {
                    if (kind == kBernoulli) {
                        fill = c.raw0[i] < 0.5 ? 0.f : 1.f;
                    } else if (kind == kCategorical) {
                        const int k0 = c.arg1[i], nk = c.arg2[i];
                        double pbest = c.cat_prob[k0];
                        int kb = 0;
                        for (int j = 1; j < nk; ++j)
                            if (c.cat_prob[k0 + j] > pbest) {
                                pbest = c.cat_prob[k0 + j];
                                kb = j;
                            }
                        fill = (float)c.cat_value[k0 + kb];
                    } else {
                        fill = (float)c.raw0[i];      // Uniform: start, Gaussian: mean
                    }
                } else {
                    const u64 slot = ctr0 + (u64)c.n_sum + 2ull * (u64)var;
                    const float u1 = counter_uniform(a.seed, slot);
                    if (kind == kBernoulli) {
                        fill = u1 < (float)c.raw0[i] ? 1.f : 0.f;
                    } else if (kind == kCategorical) {
                        const int k0 = c.arg1[i], nk = c.arg2[i];
                        float total = 0.f;
                        for (int j = 0; j < nk; ++j) total += (float)c.cat_prob[k0 + j];
                        const float target = u1 * total;
                        float cum = 0.f;
                        int kb = 0;
                        bool found = false;
                        for (int j = 0; j < nk; ++j) {
                            const float pj = (float)c.cat_prob[k0 + j];
                            cum += pj;
                            if (!found && pj > 0.f) kb = j;
                            if (!found && target < cum) {
                                kb = j;
                                found = true;
                            }
                        }
                        fill = (float)c.cat_value[k0 + kb];
                    } else if (kind == kUniform) {
                        fill = fmaf((float)c.raw1[i], u1, (float)c.raw0[i]);
                    } else {
                        const float u2 = counter_uniform(a.seed, slot + 1ull);
                        const float z = sqrtf(-2.f * logf(1.f - u1)) * cospif(2.f * u2);
                        fill = fmaf((float)c.raw1[i], z, (float)c.raw0[i]);
                    }
                }
                xrow[var] = fill;       // (mine implies own)
            }
        }
    }
}

// parents before children over column b of the tables (row = node id, row stride B)
__device__ __forceinline__ void backward_column(const Circuit &c, const float *lls, float *grads, int64_t B, int64_t b) {
    const int n = c.n_nodes;
    for (int t = 0; t < n; ++t) {
        const int i = c.order[t];
        grads[(int64_t)i * B + b] = (i == c.root) ? 0.f : -INFINITY;
    }
    for (int t = n - 1; t >= 0; --t) {
        const int i = c.order[t];
        const int kind = c.kind[i];
        if (kind != kSum && kind != kProduct) continue;
        const int c0 = c.arg0[i], nc = c.arg1[i];
        const float g = grads[(int64_t)i * B + b];
        if (kind == kSum) {
            for (int j = 0; j < nc; ++j) {
                float *dst = grads + (int64_t)c.child_index[c0 + j] * B + b;
                *dst = log_add_exp(*dst, g + c.child_logw[c0 + j]);
            }
        } else {
            const float gv = g + lls[(int64_t)i * B + b];
            for (int j = 0; j < nc; ++j) {
                const int64_t o = (int64_t)c.child_index[c0 + j] * B + b;
                grads[o] = log_add_exp(grads[o], gv - lls[o]);
            }
        }
    }
}

__global__ __launch_bounds__(64) void flat_backward_kernel(const Circuit c, const float *lls, float *grads, int64_t B) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    backward_column(c, lls, grads, B, b);
}

struct EmArgs {
    Circuit c;
    const float *x;
    int64_t N, Bb;
    int D;
    const int32_t *index;
    float *lls, *grads;
    double *utmp;       // [n_child]
    double *mean_ll;
    double eta;
};

__device__ __forceinline__ const float *em_row(const EmArgs &a, int64_t b) {
    int64_t r = a.index[b];
    r = r < 0 ? 0 : (r >= a.N ? a.N - 1 : r);
    return a.x + r * a.D;
}

__global__ __launch_bounds__(64) void flat_em_tables_kernel(const EmArgs a) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= a.Bb) return;
    const Circuit &c = a.c;
    const float *xrow = em_row(a, b);
    auto load = [&](int row) -> float { return a.lls[(int64_t)row * a.Bb + b]; };
    for (int t = 0; t < c.n_nodes; ++t) {
        const int i = c.order[t];
        a.lls[(int64_t)i * a.Bb + b] = node_value(c, i, c.kind[i], xrow, c.child_index, load);
    }
    backward_column(c, a.lls, a.grads, a.Bb, b);
}

// sum over the work-group in a fixed order, result in every thread (red: 4 doubles)
__device__ __forceinline__ double block_sum_f64(double v, double *red) {
    v = wave_reduce_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kUpdThreads) void flat_em_update_kernel(const EmArgs a) {
    __shared__ double red[4];
    const Circuit &c = a.c;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int64_t Bb = a.Bb;
    const float *R = a.lls + (int64_t)c.root * Bb;
    if (i == c.n_nodes) {       // batch mean of the root's log-likelihood
        double acc = 0.0;
        for (int64_t b = tid; b < Bb; b += kUpdThreads) acc += (double)R[b];
        const double s = block_sum_f64(acc, red);
        if (tid == 0 && a.mean_ll) *a.mean_ll = s / (double)Bb;
        return;
    }
    const int kind = c.kind[i];
    if (kind == kProduct || kind == kUniform) return;
    const double eta = a.eta, eps = 1.1920928955078125e-07 /* float32 eps */, alpha = 0.0009765625 /* float16 eps */;
    const float *L = a.lls + (int64_t)i * Bb, *G = a.grads + (int64_t)i * Bb;
    if (kind == kSum) {             // node.py:100-111
        const int c0 = c.arg0[i], nc = c.arg1[i];
        double usum = 0.0;
        for (int k = 0; k < nc; ++k) {
            const float *Lc = a.lls + (int64_t)c.child_index[c0 + k] * Bb;
            double acc = 0.0;
            for (int64_t b = tid; b < Bb; b += kUpdThreads) acc += (double)expf(Lc[b] - R[b] + G[b]);
            const double S = block_sum_f64(acc, red);
            const double u = (double)c.child_weight[c0 + k] * S + eps;
            usum += u;
            if (tid == 0) a.utmp[c0 + k] = u;
        }
        if (tid == 0)
            for (int k = 0; k < nc; ++k) {
                const float w = (float)((1.0 - eta) * (double)c.child_weight[c0 + k] + eta * (a.utmp[c0 + k] / usum));
                c.child_weight[c0 + k] = w;
                c.child_logw[c0 + k] = logf(w);
            }
        return;
    }
    const int var = c.arg0[i];
    double accT = 0.0, accA = 0.0;
    for (int64_t b = tid; b < Bb; b += kUpdThreads) {
        const double s = (double)expf(L[b] - R[b] + G[b]);
        accT += s;
        accA += s * (double)em_row(a, b)[var];
    }
    const double T = block_sum_f64(accT, red);
    if (kind == kBernoulli) {       // leaf.py:167-174
        const double A = block_sum_f64(accA, red);
        if (tid == 0) {
            const double p = (1.0 - eta) * c.raw0[i] + eta * ((A + alpha) / (T + 2.0 * alpha));
            c.raw0[i] = p;
            c.par0[i] = p > 0.0 ? log(p) : -INFINITY;
            c.par1[i] = p < 1.0 ? log1p(-p) : -INFINITY;
        }
    } else if (kind == kCategorical) {      // leaf.py:281-293
        const int k0 = c.arg1[i], nk = c.arg2[i];
        for (int k = 0; k < nk; ++k) {
            const float cv = (float)c.cat_value[k0 + k];
            double acc = 0.0;
            for (int64_t b = tid; b < Bb; b += kUpdThreads)
                if (em_row(a, b)[var] == cv) acc += (double)expf(L[b] - R[b] + G[b]);
            const double A = block_sum_f64(acc, red);
            if (tid == 0) {
                const double p = (1.0 - eta) * c.cat_prob[k0 + k] + eta * ((A + alpha) / (T + (double)nk * alpha));
                c.cat_prob[k0 + k] = p;
                c.cat_logp[k0 + k] = (float)log(p);
            }
        }
    } else {                        // Gaussian, leaf.py:536-545; second moment centred on the new mean
        const double A = block_sum_f64(accA, red);
        const double Tp = T + eps, m = A / Tp;
        double acc = 0.0;
        for (int64_t b = tid; b < Bb; b += kUpdThreads) {
            const double d = (double)em_row(a, b)[var] - m;
            acc += (double)expf(L[b] - R[b] + G[b]) * d * d;
        }
        const double V = block_sum_f64(acc, red);
        if (tid == 0) {
            const double sd = fmax(sqrt(V / Tp), 1e-5);
            const double mean = (1.0 - eta) * c.raw0[i] + eta * m, stddev = (1.0 - eta) * c.raw1[i] + eta * sd;
            c.raw0[i] = mean;
            c.raw1[i] = stddev;
            c.par0[i] = mean;
            c.par1[i] = stddev;
        }
    }
}

static inline bool topdown_lds_fits(const Circuit &c) {
    return c.n_slots > 0 && (int64_t)c.n_slots * 256 + (int64_t)c.n_nodes * 8 + (int64_t)c.n_sum * 64 <= kLdsBytes;
}
static inline int64_t topdown_lds_bytes(const Circuit &c) {
    return (int64_t)c.n_slots * 256 + (int64_t)c.n_nodes * 8 + (int64_t)c.n_sum * 64;
}
static int check_circuit(const Circuit *c, const char *what) {
    DPK_REQUIRE(c != nullptr, DPK_EINVAL, "%s: null circuit", what);
    DPK_REQUIRE(c->n_nodes > 0 && c->root >= 0 && c->root < c->n_nodes && c->n_sum >= 0 && c->n_vars > 0 && c->n_child > 0 &&
                    c->n_cat > 0 && c->n_slots >= 0,
                DPK_EINVAL, "%s: bad sizes", what);
    DPK_REQUIRE(c->order && c->kind && c->arg0 && c->arg1 && c->arg2 && c->sum_index && c->child_index && c->child_slot &&
                    c->node_slot && c->cat_value && c->child_weight && c->child_logw && c->cat_logp && c->par0 && c->par1 &&
                    c->raw0 && c->raw1 && c->cat_prob,
                DPK_EINVAL, "%s: null node arrays", what);
    return DPK_OK;
}

}  // namespace fq
}  // namespace dpk

using namespace dpk;
using namespace dpk::fq;

extern "C" int64_t dpk_flat_spn_topdown_workspace_bytes(int64_t B, const dpk_flat_spn_circuit *c) {
    if (B < 0 || c == nullptr || c->n_nodes <= 0 || c->n_sum < 0 || c->n_slots < 0) return DPK_EINVAL;
    if (topdown_lds_fits(*c)) return 0;
    const int64_t waves = (B + 63) / 64;
    return align_up((int64_t)c->n_nodes * B * 4, 256) + align_up((int64_t)c->n_sum * B, 256) +
           align_up(waves * c->n_nodes * 8, 256) + 256;
}

extern "C" int dpk_flat_spn_topdown(float *x, int64_t B, int32_t D, const dpk_flat_spn_circuit *c, int32_t mode,
                                    uint64_t seed, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = check_circuit(c, "flat_spn_topdown")) return rc;
    DPK_REQUIRE(B >= 0 && D >= c->n_vars && (mode == 0 || mode == 1), DPK_EINVAL, "flat_spn_topdown: bad sizes");
    DPK_REQUIRE(c->max_children >= 0 && c->max_children <= 255, DPK_EUNSUPPORTED,
                "flat_spn_topdown: a sum node with %d children (the branch is kept in one byte)", (int)c->max_children);
    if (B == 0) return DPK_OK;
    DPK_REQUIRE(x != nullptr, DPK_EINVAL, "flat_spn_topdown: null pointer");
    TopdownArgs a{};
    a.c = *c; a.x = x; a.B = B; a.D = D; a.n_slots = c->n_slots; a.seed = seed;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)cdiv(B, 64);
    if (topdown_lds_fits(*c)) {
        const size_t lds = (size_t)topdown_lds_bytes(*c);
        if (mode == 0)
            DPK_LAUNCH("flat_spn_topdown", (flat_topdown_kernel<true, false>), dim3(blocks), dim3(64), lds, st, a);
        else
            DPK_LAUNCH("flat_spn_topdown", (flat_topdown_kernel<true, true>), dim3(blocks), dim3(64), lds, st, a);
    } else {
        const int64_t need = dpk_flat_spn_topdown_workspace_bytes(B, c);
        DPK_REQUIRE(ws && ws_bytes >= need, DPK_EWORKSPACE, "flat_spn_topdown: workspace %lld < %lld", (long long)ws_bytes,
                    (long long)need);
        char *p = (char *)ws;
        a.table = (float *)p;
        p += align_up((int64_t)c->n_nodes * B * 4, 256);
        a.branch = (unsigned char *)p;
        p += align_up((int64_t)c->n_sum * B, 256);
        a.reach = (u64 *)p;
        if (mode == 0)
            DPK_LAUNCH("flat_spn_topdown", (flat_topdown_kernel<false, false>), dim3(blocks), dim3(64), 0, st, a);
        else
            DPK_LAUNCH("flat_spn_topdown", (flat_topdown_kernel<false, true>), dim3(blocks), dim3(64), 0, st, a);
    }
    return DPK_OK;
}

extern "C" int dpk_flat_spn_backward(const float *lls, float *grads, int64_t B, const dpk_flat_spn_circuit *c, void *stream) {
    if (int rc = check_circuit(c, "flat_spn_backward")) return rc;
    DPK_REQUIRE(B >= 0, DPK_EINVAL, "flat_spn_backward: bad sizes");
    if (B == 0) return DPK_OK;
    DPK_REQUIRE(lls && grads, DPK_EINVAL, "flat_spn_backward: null pointer");
    DPK_LAUNCH("flat_spn_backward", flat_backward_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream,
               *c, lls, grads, B);
    return DPK_OK;
}

extern "C" int64_t dpk_flat_spn_em_step_workspace_bytes(int64_t B, const dpk_flat_spn_circuit *c) {
    if (B < 0 || c == nullptr || c->n_nodes <= 0 || c->n_child <= 0) return DPK_EINVAL;
    return 2 * align_up((int64_t)c->n_nodes * B * 4, 256) + align_up((int64_t)c->n_child * 8, 256);
}

extern "C" int dpk_flat_spn_em_step(const float *x, int64_t N, int32_t D, const int32_t *index, int64_t B,
                                    const dpk_flat_spn_circuit *c, double step_size, double *mean_ll, void *ws,
                                    int64_t ws_bytes, void *stream) {
    if (int rc = check_circuit(c, "flat_spn_em_step")) return rc;
    DPK_REQUIRE(B >= 0 && N >= 0 && D >= c->n_vars && step_size > 0.0 && step_size < 1.0, DPK_EINVAL,
                "flat_spn_em_step: bad sizes");
    if (B == 0) return DPK_OK;
    DPK_REQUIRE(x && index && N > 0, DPK_EINVAL, "flat_spn_em_step: null pointer");
    const int64_t need = dpk_flat_spn_em_step_workspace_bytes(B, c);
    DPK_REQUIRE(ws && ws_bytes >= need, DPK_EWORKSPACE, "flat_spn_em_step: workspace %lld < %lld", (long long)ws_bytes,
                (long long)need);
    EmArgs a{};
    a.c = *c; a.x = x; a.N = N; a.Bb = B; a.D = D; a.index = index; a.eta = step_size; a.mean_ll = mean_ll;
    char *p = (char *)ws;
    const int64_t tab = align_up((int64_t)c->n_nodes * B * 4, 256);
    a.lls = (float *)p;
    a.grads = (float *)(p + tab);
    a.utmp = (double *)(p + 2 * tab);
    hipStream_t st = (hipStream_t)stream;
    DPK_LAUNCH("flat_spn_em_step (tables)", flat_em_tables_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, a);
    DPK_LAUNCH("flat_spn_em_step (update)", flat_em_update_kernel, dim3((unsigned)c->n_nodes + 1), dim3(kUpdThreads), 0,
               st, a);
    return DPK_OK;
}
