// The node functions of a node-graph SPN flattened into arrays, once: the bottom-up value of a node (flat_spn.hip,
// flat_spn_queries.hip, spnq/flat_spn_posterior.hip) and the log-add-exp of the top-down log-gradients.  Header-only and
// force-inlined like device.h: each includer compiles them under its own flags.
//
// deeprob/spn/algorithms/inference.py:94-103 (every node value clamped at -1e31, float32):
//   Sum      node.py:116-117   logsumexp(children, b = weights)
//   Product  node.py:152-153   sum(children)
//   leaves   leaf.py:182-186 (Bernoulli), :301-305 (Categorical), :475-479 (Uniform), :553-557 (Gaussian);
//            0 where the input is NaN (marginalised)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dp_device {
namespace flat {

enum : int32_t { kSum = 0, kProduct = 1, kBernoulli = 2, kCategorical = 3, kUniform = 4, kGaussian = 5 };
constexpr float kFloor = -1e31f;            // inference.py:103

// value of node i from its children's rows / its input.  Rec: any record with the arrays kind / arg0 / arg1 / arg2 / par0 /
// par1 / child_weight / cat_value / cat_logp of dpk_flat_spn_circuit (FlatSpnArgs, dpk_ and dpq_flat_spn_circuit); cidx:
// the children's rows (node ids, or slots of a recycled table); load(row): the row's value in this lane's column.
template <class Rec, class Load>
__device__ __forceinline__ float node_value(const Rec &c, int i, int kind, const float *xrow, const int32_t *cidx, Load load) {
    float v;
    if (kind == kSum) {
        // scipy logsumexp with weights: zero-weight terms are dropped, m = max of the rest (0 if not finite)
        const int c0 = c.arg0[i], nc = c.arg1[i];
        float m = -INFINITY;
        for (int j = 0; j < nc; ++j)
            if (c.child_weight[c0 + j] != 0.f) m = fmaxf(m, load(cidx[c0 + j]));
        if (!(fabsf(m) < INFINITY)) m = 0.f;
        float s = 0.f;
        for (int j = 0; j < nc; ++j) {
            const float w = c.child_weight[c0 + j];
            if (w != 0.f) s += w * expf(load(cidx[c0 + j]) - m);
        }
        v = logf(s) + m;
    } else if (kind == kProduct) {
        const int c0 = c.arg0[i], nc = c.arg1[i];
        v = 0.f;
        for (int j = 0; j < nc; ++j) v += load(cidx[c0 + j]);
    } else {
        const float xv = xrow[c.arg0[i]];
        if (xv != xv) {
            v = 0.f;
        } else if (kind == kBernoulli) {          // par0 = log p, par1 = log1p(-p)
            v = (xv == 1.f) ? (float)c.par0[i] : (xv == 0.f) ? (float)c.par1[i] : -INFINITY;
        } else if (kind == kCategorical) {        // x.astype(int64): truncation toward zero
            const int k0 = c.arg1[i], nk = c.arg2[i];
            const long long cat = (long long)xv;
            v = -INFINITY;
            for (int j = 0; j < nk; ++j)
                if ((long long)c.cat_value[k0 + j] == cat) v = c.cat_logp[k0 + j];
        } else if (kind == kUniform) {            // par0 = start, par1 = width
            const double z = ((double)xv - c.par0[i]) / c.par1[i];
            v = (z >= 0.0 && z <= 1.0) ? (float)(-log(c.par1[i])) : -INFINITY;
        } else {                                  // Gaussian: par0 = mean, par1 = stddev
            const double z = ((double)xv - c.par0[i]) / c.par1[i];
            v = (float)(-0.5 * z * z - 0.91893853320467274178 - log(c.par1[i]));
        }
    }
    return fmaxf(v, kFloor);
}

// log(exp(p) + exp(q)); all -inf stays -inf
__device__ __forceinline__ float log_add_exp(float p, float q) {
    const float m = fmaxf(p, q);
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(-fabsf(p - q)));
}

}  // namespace flat
}  // namespace dp_device
