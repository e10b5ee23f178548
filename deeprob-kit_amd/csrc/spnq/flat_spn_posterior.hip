// Posterior queries on a node-graph SPN flattened into arrays: conditional moments of the unobserved entries and the
// posterior of one discrete variable, one launch (dpq_flat_spn_posterior, include/deeprob_spnq.h -- the header states the
// identity, the three passes and the order of every sum; this file follows it statement for statement).
//
// Replaces deeprob/spn/algorithms/moments.py (the reference computes unconditional moments only: an all-NaN row) and gives
// what the reference has no function for: E[x_j^k | e] and p(x_j = v | e) under evidence.
//
// Organisation of flat_topdown_kernel (csrc/flat_spn_queries.hip): a 64-lane wave per 64 rows, lane = row, the node loop
// uniform over the wave so that node records come through wave-uniform loads, tables [node][row] so that every access
// is one 256-byte row per wave (one LDS bank per lane, no conflict).  A lane touches its own column only: there is no
// barrier and no cross-lane traffic, and a tail lane simply leaves.  The node functions are those of
// shared/flat_spn_nodes.h, the one definition flat_spn.hip and flat_spn_queries.hip use too; -ffp-contract=off
// (csrc/Makefile) keeps every product and sum as written.
#include "spnq_common.h"
#include "../shared/flat_spn_nodes.h"
#include <stddef.h>
#include "../../../include/deeprob_hip.h"

// one record serves both libraries
#define DPQ_SAME_FIELD(f)                                                                   \
    static_assert(offsetof(dpq_flat_spn_circuit, f) == offsetof(dpk_flat_spn_circuit, f) && \
                      sizeof(((dpq_flat_spn_circuit *)0)->f) == sizeof(((dpk_flat_spn_circuit *)0)->f), \
                  "dpq_flat_spn_circuit differs from dpk_flat_spn_circuit at " #f)
static_assert(sizeof(dpq_flat_spn_circuit) == sizeof(dpk_flat_spn_circuit), "dpq_flat_spn_circuit: size");
DPQ_SAME_FIELD(n_nodes); DPQ_SAME_FIELD(root); DPQ_SAME_FIELD(n_sum); DPQ_SAME_FIELD(n_vars); DPQ_SAME_FIELD(n_child);
DPQ_SAME_FIELD(n_cat); DPQ_SAME_FIELD(n_slots); DPQ_SAME_FIELD(max_children);
DPQ_SAME_FIELD(order); DPQ_SAME_FIELD(kind); DPQ_SAME_FIELD(arg0); DPQ_SAME_FIELD(arg1); DPQ_SAME_FIELD(arg2);
DPQ_SAME_FIELD(sum_index); DPQ_SAME_FIELD(child_index); DPQ_SAME_FIELD(child_slot); DPQ_SAME_FIELD(node_slot);
DPQ_SAME_FIELD(cat_value); DPQ_SAME_FIELD(child_weight); DPQ_SAME_FIELD(child_logw); DPQ_SAME_FIELD(cat_logp);
DPQ_SAME_FIELD(par0); DPQ_SAME_FIELD(par1); DPQ_SAME_FIELD(raw0); DPQ_SAME_FIELD(raw1); DPQ_SAME_FIELD(cat_prob);

namespace dpq_detail {

using namespace dp_device::flat;     // the kinds, kFloor, node_value, log_add_exp
using Circuit = dpq_flat_spn_circuit;

// non-central moments of order 1..4 of leaf i (the header's table)
__device__ __forceinline__ void leaf_moments(const Circuit &c, int i, int kind, double &m1, double &m2, double &m3, double &m4) {
    if (kind == kBernoulli) {
        m1 = m2 = m3 = m4 = c.raw0[i];
    } else if (kind == kCategorical) {
        const int k0 = c.arg1[i], nk = c.arg2[i];
        m1 = m2 = m3 = m4 = 0.0;
        for (int j = 0; j < nk; ++j) {
            const double v = (double)c.cat_value[k0 + j], p = c.cat_prob[k0 + j];
            const double v2 = v * v, v3 = v2 * v, v4 = v3 * v;
            m1 += v * p;
            m2 += v2 * p;
            m3 += v3 * p;
            m4 += v4 * p;
        }
    } else if (kind == kUniform) {
        const double s = c.raw0[i], w = c.raw1[i], b = s + w;
        const double b2 = b * b, b3 = b2 * b, b4 = b3 * b, b5 = b4 * b;
        const double s2 = s * s, s3 = s2 * s, s4 = s3 * s, s5 = s4 * s;
        m1 = (b2 - s2) / (2.0 * w);
        m2 = (b3 - s3) / (3.0 * w);
        m3 = (b4 - s4) / (4.0 * w);
        m4 = (b5 - s5) / (5.0 * w);
    } else {
        const double mu = c.raw0[i], sd = c.raw1[i];
        const double mu2 = mu * mu, var = sd * sd;
        m1 = mu;
        m2 = mu2 + var;
        m3 = mu2 * mu + 3.0 * mu * var;
        m4 = mu2 * mu2 + 6.0 * mu2 * var + 3.0 * var * var;
    }
}

// p_L(v) of leaf i
__device__ __forceinline__ double leaf_prob(const Circuit &c, int i, int kind, float v) {
    if (kind == kBernoulli) return v == 1.f ? c.raw0[i] : v == 0.f ? 1.0 - c.raw0[i] : 0.0;
    if (kind == kCategorical) {
        const int k0 = c.arg1[i], nk = c.arg2[i];
        const long long cat = (long long)v;
        double p = 0.0;
        for (int j = 0; j < nk; ++j)
            if ((long long)c.cat_value[k0 + j] == cat) p = c.cat_prob[k0 + j];
        return p;
    }
    return 0.0;
}

struct PosteriorArgs {
    Circuit c;
    const float *x;
    int64_t B;
    int D;
    const int32_t *var_leaf_off, *var_leaf;
    int mode, n_orders, var, n_values;
    const float *values;
    float *out;
    float *val, *grad;      // workspace route: [n_nodes, B] each
};

template <bool kLds>
__global__ __launch_bounds__(64) void flat_posterior_kernel(const PosteriorArgs a) {
    extern __shared__ float lds[];
    const Circuit &c = a.c;
    const int lane = threadIdx.x, n = c.n_nodes;
    const int64_t b = (int64_t)blockIdx.x * 64 + lane, B = a.B;
    if (b >= B) return;      // (a lane reads and writes its own column only)
    const float *xrow = a.x + b * a.D;
    float *gl = lds + n * 64;
    auto val = [&](int row) -> float { return kLds ? lds[row * 64 + lane] : a.val[(int64_t)row * B + b]; };
    auto grad = [&](int row) -> float { return kLds ? gl[row * 64 + lane] : a.grad[(int64_t)row * B + b]; };
    auto set_grad = [&](int row, float v) {
        if (kLds)
            gl[row * 64 + lane] = v;
        else
            a.grad[(int64_t)row * B + b] = v;
    };

    // ---- 1. bottom-up: every node keeps its row ------------------------------------------------------------------------
    for (int t = 0; t < n; ++t) {
        const int i = c.order[t];
        const float v = node_value(c, i, c.kind[i], xrow, c.child_index, val);
        if (kLds)
            lds[i * 64 + lane] = v;
        else
            a.val[(int64_t)i * B + b] = v;
    }

    // ---- 2. top-down log-gradients, parents before children --------------------------------------------------------------
    for (int i = 0; i < n; ++i) set_grad(i, i == c.root ? 0.f : -INFINITY);      // (every node id is in the order once)
    for (int t = n - 1; t >= 0; --t) {
        const int i = c.order[t];
        const int kind = c.kind[i];
        if (kind != kSum && kind != kProduct) continue;
        const int c0 = c.arg0[i], nc = c.arg1[i];
        const float g = grad(i);
        if (kind == kSum) {
            for (int j = 0; j < nc; ++j) {
                const int ch = c.child_index[c0 + j];
                set_grad(ch, log_add_exp(grad(ch), g + c.child_logw[c0 + j]));
            }
        } else {
            const float gv = g + val(i);
            for (int j = 0; j < nc; ++j) {
                const int ch = c.child_index[c0 + j];
                set_grad(ch, log_add_exp(grad(ch), gv - val(ch)));
            }
        }
    }

    // ---- 3. leaf phase -----------------------------------------------------------------------------------------------------
    const bool dead = val(c.root) <= kFloor;        // evidence of probability zero
    const float qnan = __builtin_nanf("");
    if (a.mode == DPQ_MODE_MOMENTS) {
        const int K = a.n_orders;
        const int64_t plane = B * (int64_t)a.D;
        float *orow = a.out + b * a.D;
        for (int j = 0; j < a.D; ++j) {
            const float xv = xrow[j];
            int l0 = 0, l1 = 0;
            if (j < c.n_vars) {
                l0 = a.var_leaf_off[j];
                l1 = a.var_leaf_off[j + 1];
            }
            float r1, r2, r3, r4;
            if (l1 <= l0) {                 // outside the scope: as given
                r1 = r2 = r3 = r4 = xv;
            } else if (xv == xv) {          // observed: a point mass
                r1 = xv;
                r2 = r1 * xv;
                r3 = r2 * xv;
                r4 = r3 * xv;
            } else if (dead) {
                r1 = r2 = r3 = r4 = qnan;
            } else {
                float M = -INFINITY;
                for (int l = l0; l < l1; ++l) M = fmaxf(M, grad(a.var_leaf[l]));
                double Z = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
                for (int l = l0; l < l1; ++l) {
                    const int i = a.var_leaf[l];
                    const double e = (double)expf(grad(i) - M);
                    double m1, m2, m3, m4;
                    leaf_moments(c, i, c.kind[i], m1, m2, m3, m4);
                    Z += e;
                    s1 += e * m1;
                    s2 += e * m2;
                    s3 += e * m3;
                    s4 += e * m4;
                }
                r1 = (float)(s1 / Z);
                r2 = (float)(s2 / Z);
                r3 = (float)(s3 / Z);
                r4 = (float)(s4 / Z);
            }
            orow[j] = r1;
            if (K > 1) orow[plane + j] = r2;
            if (K > 2) orow[2 * plane + j] = r3;
            if (K > 3) orow[3 * plane + j] = r4;
        }
    } else {
        const int V = a.n_values;
        float *orow = a.out + b * (int64_t)V;
        const float xv = xrow[a.var];
        const int l0 = a.var_leaf_off[a.var], l1 = a.var_leaf_off[a.var + 1];
        if (dead) {
            for (int v = 0; v < V; ++v) orow[v] = qnan;
        } else if (xv == xv) {
            for (int v = 0; v < V; ++v) orow[v] = a.values[v] == xv ? 1.f : 0.f;
        } else {
            float M = -INFINITY;
            for (int l = l0; l < l1; ++l) M = fmaxf(M, grad(a.var_leaf[l]));
            double Z = 0.0;
            for (int l = l0; l < l1; ++l) Z += (double)expf(grad(a.var_leaf[l]) - M);
            for (int v = 0; v < V; ++v) {
                const float value = a.values[v];
                double s = 0.0;
                for (int l = l0; l < l1; ++l) {
                    const int i = a.var_leaf[l];
                    s += (double)expf(grad(i) - M) * leaf_prob(c, i, c.kind[i], value);
                }
                orow[v] = (float)(s / Z);
            }
        }
    }
}

static inline bool lds_fits(const Circuit &c, uint32_t flags) {
    return !(flags & DPQ_FLAG_FORCE_WORKSPACE) && (int64_t)c.n_nodes * 512 <= DPQ_LDS_BUDGET_BYTES;
}

static int check_circuit(const Circuit *c, const char *what) {
    DPQ_REQUIRE(c != nullptr, DPQ_EINVAL, "%s: null circuit", what);
    DPQ_REQUIRE(c->n_nodes > 0 && c->root >= 0 && c->root < c->n_nodes && c->n_sum >= 0 && c->n_vars > 0 && c->n_child > 0 &&
                    c->n_cat > 0,
                DPQ_EINVAL, "%s: bad sizes", what);
    DPQ_REQUIRE(c->order && c->kind && c->arg0 && c->arg1 && c->arg2 && c->child_index && c->cat_value && c->child_weight &&
                    c->child_logw && c->cat_logp && c->par0 && c->par1 && c->raw0 && c->raw1 && c->cat_prob,
                DPQ_EINVAL, "%s: null node arrays", what);
    return DPQ_OK;
}

}  // namespace dpq_detail

using namespace dpq_detail;

extern "C" const char *dpq_last_error(void) { return g_error; }
extern "C" int dpq_abi_version(void) { return 1; }

extern "C" int64_t dpq_flat_spn_posterior_workspace_bytes(int64_t B, const dpq_flat_spn_circuit *c, uint32_t flags) {
    DPQ_REQUIRE(B >= 0 && c != nullptr && c->n_nodes > 0, DPQ_EINVAL, "flat_spn_posterior_workspace_bytes: bad sizes");
    if (lds_fits(*c, flags)) return 0;
    return 2 * align_up((int64_t)c->n_nodes * B * 4, 256);
}

extern "C" int dpq_flat_spn_posterior(const float *x, int64_t B, int32_t D, const dpq_flat_spn_circuit *c,
                                      const int32_t *var_leaf_off, const int32_t *var_leaf, int32_t n_leaves, int32_t mode,
                                      int32_t n_orders, int32_t var, const float *values, int32_t n_values, float *out,
                                      uint32_t flags, void *ws, int64_t ws_bytes, void *stream) {
    if (int rc = check_circuit(c, "flat_spn_posterior")) return rc;
    DPQ_REQUIRE(B >= 0 && D >= c->n_vars && n_leaves > 0, DPQ_EINVAL, "flat_spn_posterior: bad sizes");
    DPQ_REQUIRE(mode == DPQ_MODE_MOMENTS || mode == DPQ_MODE_VALUES, DPQ_EINVAL, "flat_spn_posterior: mode %d", (int)mode);
    DPQ_REQUIRE((flags & ~DPQ_FLAG_FORCE_WORKSPACE) == 0u, DPQ_EINVAL, "flat_spn_posterior: unknown flags %u", (unsigned)flags);
    if (mode == DPQ_MODE_MOMENTS)
        DPQ_REQUIRE(n_orders >= 1 && n_orders <= DPQ_MAX_ORDERS, DPQ_EINVAL, "flat_spn_posterior: %d orders (1 .. %d)",
                    (int)n_orders, DPQ_MAX_ORDERS);
    else
        DPQ_REQUIRE(var >= 0 && var < c->n_vars && n_values >= 1, DPQ_EINVAL,
                    "flat_spn_posterior: variable %d of %d, %d values", (int)var, (int)c->n_vars, (int)n_values);
    if (B == 0) return DPQ_OK;
    DPQ_REQUIRE(x && out && var_leaf_off && var_leaf && (mode == DPQ_MODE_MOMENTS || values), DPQ_EINVAL,
                "flat_spn_posterior: null pointer");
    PosteriorArgs a{};
    a.c = *c; a.x = x; a.B = B; a.D = D; a.var_leaf_off = var_leaf_off; a.var_leaf = var_leaf;
    a.mode = mode; a.n_orders = n_orders; a.var = var; a.n_values = n_values; a.values = values; a.out = out;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((B + 63) / 64);
    if (lds_fits(*c, flags)) {
        DPQ_LAUNCH("flat_spn_posterior", (flat_posterior_kernel<true>), dim3(blocks), dim3(64), (size_t)c->n_nodes * 512, st, a);
    } else {
        const int64_t tab = align_up((int64_t)c->n_nodes * B * 4, 256);
        DPQ_REQUIRE(ws && ws_bytes >= 2 * tab, DPQ_EWORKSPACE, "flat_spn_posterior: workspace %lld < %lld", (long long)ws_bytes,
                    (long long)(2 * tab));
        a.val = (float *)ws;
        a.grad = (float *)((char *)ws + tab);
        DPQ_LAUNCH("flat_spn_posterior", (flat_posterior_kernel<false>), dim3(blocks), dim3(64), 0, st, a);
    }
    return DPQ_OK;
}
