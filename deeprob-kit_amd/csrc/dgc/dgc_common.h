// libdeeprob_dgc.so's instance of the shared entry-point scaffolding (error text, checks, compute units), and what its two
// top-down passes (dgcspn_topdown.hip, dgcspn_moments.hip) share: a product level, its taps and values, the geometry table.
#pragma once
#include "../../../include/deeprob_dgc.h"
#define DP_ENTRY_NS dpg_detail
#define DP_ENTRY_ELAUNCH DPG_ELAUNCH
#include "../shared/entry.h"

#define DPG_REQUIRE(cond, ...) DP_REQUIRE(cond, DPG_EINVAL, __VA_ARGS__)
#define DPG_LAUNCH DP_LAUNCH

namespace dpg_detail {

struct Level {
    int cin, hin, win, cout, hout, wout, pl, pt, stride, dil, dw;
    int cin2, cin3;                  // Cin^2, Cin^3 (channel decode of a level that is not depthwise)
};

__device__ __forceinline__ int tap_channel(const Level &g, int oc, int t) {
    if (g.dw) return oc;
    const int q = t == 0 ? oc / g.cin3 : t == 1 ? oc / g.cin2 : t == 2 ? oc / g.cin : oc;
    return q % g.cin;
}

// fp32 value of product (oc, oh, ow) of level g over the sample's input map A [Cin, Hin, Win]: ((v0 + v1) + v2) + v3
__device__ __forceinline__ float prod_value(const Level &g, const float *A, int oc, int oh, int ow) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ih = oh * g.stride + (t >> 1) * g.dil - g.pt, iw = ow * g.stride + (t & 1) * g.dil - g.pl;
        float v = 0.f;
        if ((unsigned)ih < (unsigned)g.hin && (unsigned)iw < (unsigned)g.win)
            v = A[((int64_t)tap_channel(g, oc, t) * g.hin + ih) * g.win + iw];
        s = t == 0 ? v : s + v;
    }
    return s;
}

// lv[0 .. n_levels) from the rows of `geom`, checked against the limits of include/deeprob_dgc.h; `who` opens the error
// text.  K > 0: level 0 must read the leaf map [K, H, W].
inline int parse_geometry(const char *who, int n_levels, const int32_t *geom, int K, int H, int W, Level *lv) {
    DPG_REQUIRE(n_levels >= 1 && n_levels <= DPG_MAX_LEVELS, "%s: %d levels are outside 1..%d", who, n_levels, DPG_MAX_LEVELS);
    DPG_REQUIRE(geom != nullptr, "%s: null table", who);
    for (int j = 0; j < n_levels; ++j) {
        const int32_t *r = geom + (size_t)j * DPG_GEOM_INTS;
        Level &g = lv[j];
        g.cin = r[0]; g.hin = r[1]; g.win = r[2]; g.cout = r[3]; g.hout = r[4]; g.wout = r[5];
        g.pl = r[6]; g.pt = r[8]; g.stride = r[10]; g.dil = r[11]; g.dw = r[12] != 0;
        g.cin2 = g.cin3 = 0;
        DPG_REQUIRE(g.cin >= 1 && g.cin <= 32767 && g.hin >= 1 && g.win >= 1 && (int64_t)g.hin * g.win <= 65535 &&
                        g.hout >= 1 && g.wout >= 1 && (int64_t)g.hout * g.wout <= 65535 && g.stride >= 1 && g.stride <= 65535 && g.dil >= 1 &&
                        g.dil <= 65535,
                    "%s: level %d: sizes out of domain", who, j);
        // (with these bounds out * stride + dilation - pad stays far inside int)
        for (int q = 6; q < 10; ++q)
            DPG_REQUIRE(r[q] >= -65535 && r[q] <= 65535, "%s: level %d: pad %d out of domain", who, j, r[q]);
        // (the pads after a map shape its output only; they are checked through the output shape)
        const int64_t eff = (int64_t)g.dil + 1;
        const int64_t span_h = (int64_t)r[8] + r[9] + g.hin - eff + 1, span_w = (int64_t)r[6] + r[7] + g.win - eff + 1;
        DPG_REQUIRE(span_h >= 1 && span_w >= 1 && g.hout == (span_h + g.stride - 1) / g.stride &&
                        g.wout == (span_w + g.stride - 1) / g.stride,
                    "%s: level %d: the output shape does not follow from pads, stride and dilation", who, j);
        if (g.dw) {
            DPG_REQUIRE(g.cout == g.cin, "%s: level %d: depthwise with %d -> %d channels", who, j, g.cin, g.cout);
        } else {
            const int64_t c2 = (int64_t)g.cin * g.cin, c4 = c2 * c2;
            DPG_REQUIRE(g.cin <= 181 && g.cout == c4, "%s: level %d: %d channels do not give %d = Cin^4", who, j, g.cin, g.cout);
            g.cin2 = (int)c2;
            g.cin3 = (int)(c2 * g.cin);
        }
        DPG_REQUIRE((int64_t)g.cout * g.hout * g.wout <= 0x7fffffff, "%s: level %d: map too large", who, j);
        if (j == 0)
            DPG_REQUIRE(K <= 0 || (g.cin == K && g.hin == H && g.win == W), "%s: level 0 does not read the leaf map", who);
        else
            DPG_REQUIRE(g.hin == lv[j - 1].hout && g.win == lv[j - 1].wout, "%s: level %d does not read the map of level %d", who,
                        j, j - 1);
    }
    return DPG_OK;
}

}  // namespace dpg_detail
