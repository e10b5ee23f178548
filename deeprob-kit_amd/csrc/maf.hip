// Masked autoregressive flow (MAF) on gfx950: AutoregressiveLayer of deeprob/flows/layers/autoregressive.py:13-181.
//
// Three routes:
//  * Fused density kernel (apply_backward, no autograd graph), envelope: depth-1 conditioner, 1 <= units <= 256, any
//    D >= 2, the five activations.  One 256-thread work-group per 64 samples: GEMM 1 (X W1m^T, K walked in chunks of
//    64 inputs staged in LDS) and GEMM 2 (H W2m^T) on v_mfma_f32_32x32x2_f32 (exact fp32 products), hidden activations
//    in LDS, ScaledTanh + affine + log-det epilogue in registers: Z [B, 2D] never reaches HBM.  The masked weights
//    (W * M) are packed per call (maf_pack_density_kernel) in an order the caller chooses -- inputs, hidden units and
//    outputs sorted by degree -- and per 32-row tile the packed K extent that holds a non-zero mask entry is taken from
//    the LIVE mask buffers (maf_klimit_kernel): all-zero K blocks are skipped, and a mask written through `.data` is
//    seen by the next call whatever order the caller passed (the order only decides how much is skipped).
//  * Sampling kernel (apply_forward, no graph), envelope: depth 1, units <= 128, any mask.  One lane per sample
//    carries the first layer's pre-activations h = b1 + sum_{produced j} W1m[:, j] x_j through the D steps (the
//    reference evaluates the whole conditioner on the partially produced x, whose other entries are 0: for depth 1
//    that is exactly this h).  The per-step rows of W2m and column of W1m are packed in step order and staged through
//    LDS 32 steps at a time; every read of them is a broadcast.
//  * Chained route (everything else, and training): masked weights formed per call, the generic fp32-MFMA GEMM of
//    gemm_f32.h per layer, an activation pass, and the affine epilogue; its backward gives dW = M * (dOut^T In).
#include "common.h"
#include "gemm_f32.h"
#include <math.h>

namespace dpk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

enum { kActRelu = 0, kActLeaky = 1, kActSoftplus = 2, kActTanh = 3, kActSigmoid = 4 };

template <int ACT>
__device__ __forceinline__ float act_fwd(float v) {
    if constexpr (ACT == kActRelu) return fmaxf(v, 0.f);
    else if constexpr (ACT == kActLeaky) return v > 0.f ? v : 0.01f * v;
    else if constexpr (ACT == kActSoftplus) return v > 20.f ? v : log1pf(expf(v));   // nn.Softplus(beta=1, threshold=20)
    else if constexpr (ACT == kActTanh) return tanhf(v);
    else return 1.f / (1.f + expf(-v));
}
__device__ __forceinline__ float act_any(int act, float v) {
    switch (act) {
        case kActRelu: return act_fwd<kActRelu>(v);
        case kActLeaky: return act_fwd<kActLeaky>(v);
        case kActSoftplus: return act_fwd<kActSoftplus>(v);
        case kActTanh: return act_fwd<kActTanh>(v);
        default: return act_fwd<kActSigmoid>(v);
    }
}
// derivative from the activation's OUTPUT y (what the chained route keeps)
__device__ __forceinline__ float act_grad_from_out(int act, float y) {
    switch (act) {
        case kActRelu: return y > 0.f ? 1.f : 0.f;
        case kActLeaky: return y > 0.f ? 1.f : 0.01f;
        case kActSoftplus: return -expm1f(-y);          // sigmoid(x) = 1 - exp(-softplus(x))
        case kActTanh: return 1.f - y * y;
        default: return y * (1.f - y);
    }
}

static inline int grid_for(int64_t n, int block = 256, int cap = 16384) {
    const int64_t b = (n + block - 1) / block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- chained route ---------------------------------------------------------------------------------------------------
__global__ void maf_mul_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n, float *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = a[e] * b[e];
}

__global__ void maf_act_kernel(float *__restrict__ h, int64_t n, int act) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        h[e] = act_any(act, h[e]);
}

__global__ void maf_act_bwd_kernel(float *__restrict__ dh, const float *__restrict__ y, int64_t n, int act) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
        dh[e] *= act_grad_from_out(act, y[e]);
}

// u = (x - t) exp(-a tanh(s)), ildj = -sum a tanh(s): one wave per row
__global__ __launch_bounds__(256) void maf_epilogue_kernel(const float *__restrict__ x, const float *__restrict__ Z,
                                                           int64_t B, int D, const float *__restrict__ aw,
                                                           float *__restrict__ u, float *__restrict__ ildj) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float a = aw[0];
    const float *z = Z + row * 2 * D;
    float acc = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float s = a * tanhf(z[D + d]);
        u[row * D + d] = (x[row * D + d] - z[d]) * expf(-s);
        acc += s;
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) ildj[row] = -acc;
}

// backward of the epilogue: gx = gu exp(-s') (the direct path), dZ = [dt, ds], per-row partial of dL/da in `pa`
__global__ __launch_bounds__(256) void maf_epilogue_bwd_kernel(const float *__restrict__ x, const float *__restrict__ Z,
                                                               int64_t B, int D, const float *__restrict__ aw,
                                                               const float *__restrict__ gu, const float *__restrict__ gildj,
                                                               float *__restrict__ gx, float *__restrict__ dZ,
                                                               float *__restrict__ pa) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float a = aw[0];
    const float gl = gildj ? gildj[row] : 0.f;
    const float *z = Z + row * 2 * D;
    float acc = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float th = tanhf(z[D + d]), s = a * th, e = expf(-s);
        const float g = gu ? gu[row * D + d] : 0.f;
        const float uu = (x[row * D + d] - z[d]) * e;
        const float ds = -g * uu - gl;                 // dL/ds'
        gx[row * D + d] = g * e;
        dZ[row * 2 * D + d] = -g * e;
        dZ[row * 2 * D + D + d] = ds * a * (1.f - th * th);
        acc += ds * th;
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) pa[row] = acc;
}

// column sums of a row-major [M, N] matrix, in a fixed order: out[n] (= or +=) sum_m src[m, n]
__global__ __launch_bounds__(256) void maf_colsum_kernel(const float *__restrict__ src, int64_t M, int N,
                                                         float *__restrict__ out, int accumulate) {
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    float s = 0.f;
    if (n < N)
        for (int64_t m = rg; m < M; m += 4) s += src[m * N + n];
    red[rg][c] = s;
    __syncthreads();
    if (rg == 0 && n < N) {
        const float v = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        out[n] = accumulate ? out[n] + v : v;
    }
}

struct MafChain {
    int n_lin;                 // n_hidden + 1
    int widths[34];            // out widths; widths[n_lin - 1] = 2D
    int64_t wm_off[34];        // masked weights (floats) in the workspace
    int64_t h_off[34];         // activations (floats) of the hidden layers, [B, width]
    int64_t floats[3];         // workspace of the conditioner forward (weights + activations; Z goes to the caller), of
};                             // the density forward (+ Z) and of the backward (+ the gradient buffers)

static bool chain_plan(int64_t B, int D, int n_hidden, const int32_t *widths, MafChain *c) {
    if (n_hidden < 1 || n_hidden > 32 || D < 1 || B < 0 || !widths) return false;
    c->n_lin = n_hidden + 1;
    int64_t off = 0, in = D;
    for (int l = 0; l < c->n_lin; ++l) {
        const int w = (l == n_hidden) ? 2 * D : widths[l];
        if (w <= 0) return false;
        c->widths[l] = w;
        c->wm_off[l] = off;
        off += align_up((int64_t)w * in, 64);
        in = w;
    }
    for (int l = 0; l < c->n_lin; ++l) {   // hidden activations, then Z, then the backward's two gradient buffers
        if (l == n_hidden) c->floats[0] = off;
        c->h_off[l] = off;
        off += align_up(B * c->widths[l], 64);
    }
    c->floats[1] = off;
    int64_t widest = 2 * (int64_t)D;
    for (int l = 0; l < n_hidden; ++l) widest = widths[l] > widest ? widths[l] : widest;
    c->h_off[c->n_lin] = off;                       // gradient ping-pong (backward only)
    off += 2 * align_up(B * widest, 64) + align_up(B, 64);
    c->floats[2] = off;
    return true;
}

static int chain_check(const char *who, const float *x, int64_t B, int D, int n_hidden, const float *const *W,
                       const float *const *M, const float *const *b, const int32_t *widths, int act, MafChain *c) {
    DPK_REQUIRE(B >= 0 && D >= 1 && n_hidden >= 1 && n_hidden <= 32 && act >= 0 && act <= 4, DPK_EINVAL,
                "%s: bad sizes (B %lld, D %d, n_hidden %d, activation %d)", who, (long long)B, D, n_hidden, act);
    DPK_REQUIRE(W && M && b && widths && (x || B == 0), DPK_EINVAL, "%s: null pointer", who);
    for (int l = 0; l <= n_hidden; ++l) DPK_REQUIRE(W[l] && M[l] && b[l], DPK_EINVAL, "%s: null parameter %d", who, l);
    DPK_REQUIRE(chain_plan(B, D, n_hidden, widths, c), DPK_EINVAL, "%s: bad widths", who);
    return DPK_OK;
}

static int chain_room(const char *who, const MafChain &c, int mode, int64_t ws_bytes) {
    const int64_t need = c.floats[mode] * 4 + 256;
    DPK_REQUIRE(ws_bytes >= need, DPK_EWORKSPACE, "%s: workspace %lld < %lld", who, (long long)ws_bytes, (long long)need);
    return DPK_OK;
}

// masked weights of every layer, then H_l = act(H_{l-1} Wm_l^T + b_l), Z = H_L Wm^T + b (into zout when given)
static int chain_forward(const MafChain &c, float *base, const float *x, int64_t B, int D, const float *const *W,
                         const float *const *M, const float *const *b, int act, hipStream_t st, float *zout = nullptr) {
    int in = D;
    for (int l = 0; l < c.n_lin; ++l) {
        const int64_t n = (int64_t)c.widths[l] * in;
        DPK_LAUNCH("maf_mul_kernel", maf_mul_kernel, dim3(grid_for(n)), dim3(256), 0, st, W[l], M[l], n,
                   base + c.wm_off[l]);
        in = c.widths[l];
    }
    const float *A = x;
    in = D;
    for (int l = 0; l < c.n_lin; ++l) {
        GemmArgs g{};
        g.A = A; g.sam = in; g.sak = 1;
        g.Bm = base + c.wm_off[l]; g.sbk = 1; g.sbn = in;
        g.C = (zout && l + 1 == c.n_lin) ? zout : base + c.h_off[l]; g.ldc = c.widths[l];
        g.M = (int)B; g.N = c.widths[l]; g.K = in; g.bias = b[l];
        DPK_TRY(launch_gemm(g, st));
        if (l + 1 < c.n_lin) {
            const int64_t n = B * c.widths[l];
            DPK_LAUNCH("maf_act_kernel", maf_act_kernel, dim3(grid_for(n)), dim3(256), 0, st, base + c.h_off[l], n,
                       act);
        }
        A = base + c.h_off[l];
        in = c.widths[l];
    }
    return DPK_OK;
}

// ---- fused density kernel --------------------------------------------------------------------------------------------
constexpr int kFRows = 64;      // samples per work-group
constexpr int kFKc = 64;        // inputs staged per chunk

struct DensityPack {
    int D, U, UP, HT, OT, KP;   // KP: inputs padded to kFKc; UP: units padded to 32
    int64_t w1, w2t, w2s, b1, b2t, b2s, lim1, lim2;   // float offsets in the workspace (lims are int32)
    int64_t floats;
};
static DensityPack density_pack(int D, int U) {
    DensityPack p{};
    p.D = D; p.U = U; p.UP = (int)align_up(U, 32); p.HT = p.UP / 32; p.OT = cdiv(D, 32); p.KP = (int)align_up(D, kFKc);
    int64_t o = 0;
    p.w1 = o; o += (int64_t)p.HT * 32 * p.KP;
    p.w2t = o; o += (int64_t)p.OT * 32 * p.UP;
    p.w2s = o; o += (int64_t)p.OT * 32 * p.UP;
    p.b1 = o; o += p.UP;
    p.b2t = o; o += p.OT * 32;
    p.b2s = o; o += p.OT * 32;
    p.lim1 = o; o += align_up(p.HT, 4);
    p.lim2 = o; o += align_up(p.OT, 4);
    p.floats = align_up(o, 64);
    return p;
}

// packed MFMA B fragments: tile t, k-group k8 (8 consecutive packed k), lane l, element j (0..3) holds
// Wm[row = perm_r[t*32 + (l & 31)]][col = perm_k[k8*8 + 2j + (l >> 5)]]: one 16-byte load per lane feeds 4 MFMAs
__device__ __forceinline__ int64_t frag_index(int t, int nk8, int k8, int lane, int j) {
    return (((int64_t)t * nk8 + k8) * 64 + lane) * 4 + j;
}

__global__ void maf_pack_density_kernel(DensityPack p, const float *__restrict__ W1, const float *__restrict__ M1,
                                        const float *__restrict__ b1, const float *__restrict__ W2,
                                        const float *__restrict__ M2, const float *__restrict__ b2,
                                        const int *__restrict__ iperm, const int *__restrict__ hperm,
                                        const int *__restrict__ operm, float *__restrict__ ws) {
    const int64_t n1 = (int64_t)p.HT * 32 * p.KP, n2 = (int64_t)p.OT * 32 * p.UP;
    const int64_t total = n1 + 2 * n2 + p.UP + 2 * p.OT * 32;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < n1) {
            const int j = (int)(e & 3), lane = (int)((e >> 2) & 63);
            const int64_t q = e >> 8;
            const int nk8 = p.KP / 8, k8 = (int)(q % nk8), t = (int)(q / nk8);
            const int r = t * 32 + (lane & 31), k = k8 * 8 + 2 * j + (lane >> 5);
            float v = 0.f;
            if (r < p.U && k < p.D) {
                const int64_t src = (int64_t)hperm[r] * p.D + iperm[k];
                v = W1[src] * M1[src];
            }
            ws[p.w1 + e] = v;
        } else if (e < n1 + 2 * n2) {
            const int64_t e2 = (e - n1) % n2;
            const int half = (int)((e - n1) / n2);          // 0: translation rows, 1: scale rows
            const int j = (int)(e2 & 3), lane = (int)((e2 >> 2) & 63);
            const int64_t q = e2 >> 8;
            const int nk8 = p.UP / 8, k8 = (int)(q % nk8), t = (int)(q / nk8);
            const int r = t * 32 + (lane & 31), k = k8 * 8 + 2 * j + (lane >> 5);
            float v = 0.f;
            if (r < p.D && k < p.U) {
                const int64_t src = ((int64_t)operm[r] + (int64_t)half * p.D) * p.U + hperm[k];
                v = W2[src] * M2[src];
            }
            ws[(half ? p.w2s : p.w2t) + e2] = v;
        } else if (e < n1 + 2 * n2 + p.UP) {
            const int r = (int)(e - n1 - 2 * n2);
            ws[p.b1 + r] = r < p.U ? b1[hperm[r]] : 0.f;
        } else {
            const int64_t e3 = e - n1 - 2 * n2 - p.UP;
            const int half = (int)(e3 / (p.OT * 32)), r = (int)(e3 % (p.OT * 32));
            ws[(half ? p.b2s : p.b2t) + r] = r < p.D ? b2[operm[r] + half * p.D] : 0.f;
        }
    }
}

// per 32-row tile: the number of 8-wide packed K groups up to the last one holding a non-zero mask entry
// (blocks [0, HT): first layer, [HT, HT + OT): output layer, translation and scale rows together)
__global__ __launch_bounds__(256) void maf_klimit_kernel(DensityPack p, const float *__restrict__ M1,
                                                         const float *__restrict__ M2, const int *__restrict__ iperm,
                                                         const int *__restrict__ hperm, const int *__restrict__ operm,
                                                         float *__restrict__ ws) {
    __shared__ int red[256];
    const bool first = (int)blockIdx.x < p.HT;
    const int t = first ? blockIdx.x : blockIdx.x - p.HT;
    const int K = first ? p.D : p.U, nr = first ? p.U : p.D;
    int best = 0;
    for (int64_t e = threadIdx.x; e < (int64_t)32 * K; e += 256) {
        const int r = t * 32 + (int)(e / K), k = (int)(e % K);
        if (r >= nr) continue;
        bool nz;
        if (first) {
            nz = M1[(int64_t)hperm[r] * p.D + iperm[k]] != 0.f;
        } else {
            const int64_t row = operm[r];
            nz = M2[row * p.U + hperm[k]] != 0.f || M2[(row + p.D) * p.U + hperm[k]] != 0.f;
        }
        if (nz) best = max(best, k / 8 + 1);
    }
    red[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) ((int *)(ws + (first ? p.lim1 : p.lim2)))[t] = red[0];
}

// NHT: hidden tiles per wave (units <= 128: 1, <= 256: 2)
template <int ACT, int NHT>
__global__ __launch_bounds__(256) void maf_density_kernel(DensityPack p, const float *__restrict__ x, int64_t B,
                                                          const float *__restrict__ ws, const int *__restrict__ iperm,
                                                          const int *__restrict__ operm, const float *__restrict__ aw,
                                                          const float *__restrict__ in_scale,
                                                          const float *__restrict__ in_shift, float *__restrict__ out,
                                                          float *__restrict__ ildj, int accumulate) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * kFRows;
    const int D = p.D, HS = p.UP + 1;            // (odd row strides: the 32 rows of an operand read hit distinct banks)
    float *Xs = smem;                            // [64][kFKc + 1]   (phase 1)
    float *Hs = smem;                            // [64][UP + 1]     (phase 2, over Xs)
    float *red = smem + 64 * (HS > kFKc + 1 ? HS : kFKc + 1);   // [4][64]
    const int *lim1 = (const int *)(ws + p.lim1), *lim2 = (const int *)(ws + p.lim2);
    int kmax = 0;
    for (int t = 0; t < p.HT; ++t) kmax = max(kmax, lim1[t]);
    kmax *= 8;

    f32x16 acc[NHT][2];
#pragma unroll
    for (int n = 0; n < NHT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][0][r] = acc[n][1][r] = 0.f;
    const float4 *W1f = (const float4 *)(ws + p.w1);
    const int nk8_1 = p.KP / 8;
    for (int kc = 0; kc < kmax; kc += kFKc) {
        __syncthreads();
        {
            const int c = tid & 63, k = kc + c;
            const int col = k < D ? iperm[k] : 0;
            const float sc = (in_scale && k < D) ? in_scale[col] : 1.f, sh = (in_shift && k < D) ? in_shift[col] : 0.f;
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const int r = (tid >> 6) + 4 * i;
                const int64_t b = b0 + r;
                float v = 0.f;
                if (k < D && b < B) v = x[b * D + col] * sc + sh;
                Xs[r * (kFKc + 1) + c] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NHT; ++n) {
            const int ht = wave + 4 * n;
            if (ht >= p.HT) continue;
            const int lim = min(lim1[ht] * 8, kc + kFKc);
            for (int k = kc; k < lim; k += 8) {
                const float4 bv = W1f[((int64_t)ht * nk8_1 + k / 8) * 64 + lane];
                const float bj[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kk = k - kc + 2 * j + hi;
                    const float a0 = Xs[l31 * (kFKc + 1) + kk], a1 = Xs[(32 + l31) * (kFKc + 1) + kk];
                    acc[n][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bj[j], acc[n][0], 0, 0, 0);
                    acc[n][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bj[j], acc[n][1], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();
    // hidden activations into LDS (sorted hidden order; padded units carry zero weights behind them)
#pragma unroll
    for (int n = 0; n < NHT; ++n) {
        const int ht = wave + 4 * n;
        if (ht >= p.HT) continue;
        const int col = ht * 32 + l31;
        const float bb = ws[p.b1 + col];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = h * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                Hs[m * HS + col] = act_fwd<ACT>(acc[n][h][r] + bb);
            }
    }
    __syncthreads();

    const float a = aw[0];
    float ps[2][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ps[0][r] = ps[1][r] = 0.f;
    const float4 *W2t = (const float4 *)(ws + p.w2t), *W2s = (const float4 *)(ws + p.w2s);
    const int nk8_2 = p.UP / 8;
    for (int ot = wave; ot < p.OT; ot += 4) {
        f32x16 at[2], as[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) at[0][r] = at[1][r] = as[0][r] = as[1][r] = 0.f;
        const int lim = lim2[ot] * 8;
        for (int k = 0; k < lim; k += 8) {
            const int64_t fi = ((int64_t)ot * nk8_2 + k / 8) * 64 + lane;
            const float4 tv = W2t[fi], sv = W2s[fi];
            const float tj[4] = {tv.x, tv.y, tv.z, tv.w}, sj[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + 2 * j + hi;
                const float a0 = Hs[l31 * HS + kk], a1 = Hs[(32 + l31) * HS + kk];
                at[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, tj[j], at[0], 0, 0, 0);
                at[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, tj[j], at[1], 0, 0, 0);
                as[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, sj[j], as[0], 0, 0, 0);
                as[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, sj[j], as[1], 0, 0, 0);
            }
        }
        const int n = ot * 32 + l31;
        if (n < D) {
            const int d = operm[n];
            const float bt = ws[p.b2t + n], bs = ws[p.b2s + n];
            const float sc = in_scale ? in_scale[d] : 1.f, sh = in_shift ? in_shift[d] : 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t b = b0 + h * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (b < B) {
                        const float s = a * tanhf(as[h][r] + bs), t = at[h][r] + bt;
                        out[b * D + d] = (x[b * D + d] * sc + sh - t) * expf(-s);
                        ps[h][r] -= s;
                    }
                }
        }
    }
    // per-row log-det: over the 32 lanes of a half-wave, then over the 4 waves
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = ps[h][r];
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
            if (l31 == 0) red[wave * 64 + h * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi] = v;
        }
    __syncthreads();
    if (tid < 64 && b0 + tid < B) {
        const float v = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
        ildj[b0 + tid] = accumulate ? ildj[b0 + tid] + v : v;
    }
}

// ---- sampling kernel -------------------------------------------------------------------------------------------------
constexpr int kSSteps = 32;     // steps staged in LDS at a time
constexpr int kSThreads = 256;  // samples per work-group (one per lane)

struct SamplePack {
    int D, U, UP;
    int64_t steps, bias, nz, b1, floats;   // steps: [D][3][UP] (W2m translation row, W2m scale row, W1m column) in step order
};
static SamplePack sample_pack(int D, int U) {
    SamplePack p{};
    p.D = D; p.U = U; p.UP = (int)align_up(U, 32);
    int64_t o = 0;
    p.steps = o; o += (int64_t)D * 3 * p.UP;
    p.bias = o; o += align_up(2 * (int64_t)D, 4);       // [D][2] translation / scale bias in step order
    p.nz = o; o += align_up(D, 4);                      // [D] int: W1m column non-zero
    p.b1 = o; o += p.UP;                                // b1 (padded)
    p.floats = align_up(o, 64);
    return p;
}

__global__ void maf_pack_sample_kernel(SamplePack p, const float *__restrict__ W1, const float *__restrict__ M1,
                                       const float *__restrict__ b1, const float *__restrict__ W2,
                                       const float *__restrict__ M2, const float *__restrict__ b2,
                                       const int *__restrict__ order, float *__restrict__ ws) {
    const int64_t n = (int64_t)p.D * 3 * p.UP;
    const int64_t total = n + 2 * (int64_t)p.D + p.UP;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < n) {
            const int j = (int)(e % p.UP), kind = (int)((e / p.UP) % 3);
            const int step = (int)(e / (3 * (int64_t)p.UP));
            const int i = order[step];
            float v = 0.f;
            if (j < p.U) {
                const int64_t src = kind == 2 ? (int64_t)j * p.D + i : ((int64_t)i + (kind ? p.D : 0)) * p.U + j;
                v = kind == 2 ? W1[src] * M1[src] : W2[src] * M2[src];
            }
            ws[p.steps + e] = v;
        } else if (e < n + 2 * (int64_t)p.D) {
            const int q = (int)(e - n), step = q >> 1, kind = q & 1;
            ws[p.bias + q] = b2[order[step] + (kind ? p.D : 0)];
        } else {
            const int j = (int)(e - n - 2 * (int64_t)p.D);
            ws[p.b1 + j] = j < p.U ? b1[j] : 0.f;
        }
    }
}

// column flags: does W1m[:, order[step]] hold a non-zero (otherwise the step leaves h unchanged)
__global__ void maf_sample_nz_kernel(SamplePack p, float *__restrict__ ws) {
    const int step = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (step >= p.D) return;
    const float *col = ws + p.steps + ((int64_t)step * 3 + 2) * p.UP;
    int nz = 0;
    for (int j = lane; j < p.UP; j += 64) nz |= col[j] != 0.f;
    nz = __any(nz);
    if (lane == 0) ((int *)(ws + p.nz))[step] = nz;
}

template <int ACT, int UP>
__global__ __launch_bounds__(kSThreads) void maf_sample_kernel(SamplePack p, const float *__restrict__ u, int64_t B,
                                                               const float *__restrict__ ws, const int *__restrict__ order,
                                                               const float *__restrict__ aw, float *__restrict__ x,
                                                               float *__restrict__ ldj) {
    __shared__ float4 stage[kSSteps * 3 * UP / 4];
    __shared__ float bias_s[kSSteps * 2];
    __shared__ int nz_s[kSSteps], ord_s[kSSteps];
    const int tid = threadIdx.x, D = p.D;
    const int64_t b = (int64_t)blockIdx.x * kSThreads + tid;
    const bool live = b < B;
    const int64_t row = live ? b : 0;
    constexpr bool kCheapAct = ACT == kActRelu || ACT == kActLeaky;
    float h[UP], av[kCheapAct ? 1 : UP];
    const float *b1 = ws + p.b1;
#pragma unroll
    for (int j = 0; j < UP; ++j) {
        h[j] = b1[j];
        if constexpr (!kCheapAct) av[j] = act_fwd<ACT>(h[j]);
    }
    const float a = aw[0];
    float acc_ldj = 0.f;
    const float4 *src = (const float4 *)(ws + p.steps);
    for (int p0 = 0; p0 < D; p0 += kSSteps) {
        const int ns = min(kSSteps, D - p0);
        __syncthreads();
        for (int e = tid; e < ns * 3 * UP / 4; e += kSThreads) stage[e] = src[(int64_t)p0 * 3 * UP / 4 + e];
        if (tid < 2 * ns) bias_s[tid] = ws[p.bias + 2 * p0 + tid];
        if (tid < ns) {
            nz_s[tid] = ((const int *)(ws + p.nz))[p0 + tid];
            ord_s[tid] = order[p0 + tid];
        }
        __syncthreads();
        for (int s = 0; s < ns; ++s) {
            const float4 *wt = stage + s * 3 * UP / 4, *wsc = wt + UP / 4, *w1 = wt + 2 * UP / 4;
            float t = bias_s[2 * s], sv = bias_s[2 * s + 1];
#pragma unroll
            for (int q = 0; q < UP / 4; ++q) {
                const float4 ct = wt[q], cs = wsc[q];
                float a0, a1, a2, a3;
                if constexpr (kCheapAct) {
                    a0 = act_fwd<ACT>(h[4 * q]); a1 = act_fwd<ACT>(h[4 * q + 1]);
                    a2 = act_fwd<ACT>(h[4 * q + 2]); a3 = act_fwd<ACT>(h[4 * q + 3]);
                } else {
                    a0 = av[4 * q]; a1 = av[4 * q + 1]; a2 = av[4 * q + 2]; a3 = av[4 * q + 3];
                }
                t = fmaf(ct.x, a0, t); t = fmaf(ct.y, a1, t); t = fmaf(ct.z, a2, t); t = fmaf(ct.w, a3, t);
                sv = fmaf(cs.x, a0, sv); sv = fmaf(cs.y, a1, sv); sv = fmaf(cs.z, a2, sv); sv = fmaf(cs.w, a3, sv);
            }
            const int i = ord_s[s];
            const float sp = a * tanhf(sv);
            const float xi = u[row * D + i] * expf(sp) + t;
            if (live) x[row * D + i] = xi;
            acc_ldj += sp;
            if (nz_s[s]) {
#pragma unroll
                for (int q = 0; q < UP / 4; ++q) {
                    const float4 c = w1[q];
                    h[4 * q] = fmaf(c.x, xi, h[4 * q]); h[4 * q + 1] = fmaf(c.y, xi, h[4 * q + 1]);
                    h[4 * q + 2] = fmaf(c.z, xi, h[4 * q + 2]); h[4 * q + 3] = fmaf(c.w, xi, h[4 * q + 3]);
                    if constexpr (!kCheapAct) {
                        av[4 * q] = act_fwd<ACT>(h[4 * q]); av[4 * q + 1] = act_fwd<ACT>(h[4 * q + 1]);
                        av[4 * q + 2] = act_fwd<ACT>(h[4 * q + 2]); av[4 * q + 3] = act_fwd<ACT>(h[4 * q + 3]);
                    }
                }
            }
        }
    }
    if (live) ldj[b] = acc_ldj;
}

template <int ACT>
static int launch_sample(Profile &prof, int UP, dim3 grid, hipStream_t st, const SamplePack &p, const float *u, int64_t B,
                         const float *ws, const int *order, const float *aw, float *x, float *ldj) {
    switch (UP) {
        case 32: DPK_LAUNCH_IN(prof, "maf_sample_kernel", (maf_sample_kernel<ACT, 32>), grid, dim3(kSThreads), 0, st, p,
            u, B, ws, order, aw, x, ldj); break;
        case 64: DPK_LAUNCH_IN(prof, "maf_sample_kernel", (maf_sample_kernel<ACT, 64>), grid, dim3(kSThreads), 0, st, p,
            u, B, ws, order, aw, x, ldj); break;
        case 96: DPK_LAUNCH_IN(prof, "maf_sample_kernel", (maf_sample_kernel<ACT, 96>), grid, dim3(kSThreads), 0, st, p,
            u, B, ws, order, aw, x, ldj); break;
        default: DPK_LAUNCH_IN(prof, "maf_sample_kernel", (maf_sample_kernel<ACT, 128>), grid, dim3(kSThreads), 0, st,
            p, u, B, ws, order, aw, x, ldj); break;
    }
    return DPK_OK;
}

template <int ACT>
static int launch_density(Profile &prof, int nht, const DensityPack &p, dim3 grid, int lds, hipStream_t st, const float *x, int64_t B,
                          const float *ws, const int *iperm, const int *operm, const float *aw, const float *sc,
                          const float *sh, float *out, float *ildj, int accumulate) {
    const void *k = nht == 1 ? (const void *)maf_density_kernel<ACT, 1> : (const void *)maf_density_kernel<ACT, 2>;
    DPK_TRY(ensure_dynamic_lds(k, lds));
    if (nht == 1)
        DPK_LAUNCH_IN(prof, "maf_density_kernel", (maf_density_kernel<ACT, 1>), grid, dim3(256), lds, st, p, x, B, ws,
                      iperm, operm, aw, sc, sh, out, ildj, accumulate);
    else
        DPK_LAUNCH_IN(prof, "maf_density_kernel", (maf_density_kernel<ACT, 2>), grid, dim3(256), lds, st, p, x, B, ws,
                      iperm, operm, aw, sc, sh, out, ildj, accumulate);
    return DPK_OK;
}

// ---- sampling kernel, depth >= 2 ---------------------------------------------------------------------------------------
// Masks autoregressive in the layer's order: every hidden unit becomes final at a known step (the latest step among the
// variables it depends on; the host derives it from the mask buffers).  One lane per sample keeps every hidden layer's
// pre-activations in its own LDS column; the first layer takes W1m[:, i] x_i after each step, and a unit that has
// become final is propagated ONCE into the next layer (W_{l+1}m[:, j] act(h_j)), or, in the last hidden layer, replaced
// by its activation, which the outputs read.  A unit feeding output i is final before step p(i) (that is what
// "autoregressive" is checked for), so every output sees exactly the values the reference's full conditioner gives on
// the partially produced x.  Events: event_ptr [D + 2] (slot 0: units final before any step, slot p + 1: after step p),
// events = (layer << 16) | unit, sorted by layer within a slot.
constexpr int kDeepMaxHidden = 8;
constexpr int kDeepMaxUnits = 512;          // sum of the hidden widths: 64 lanes x 512 x 4 B = 128 KB of LDS

struct DeepArgs {
    int D, L, act, total;
    int U[kDeepMaxHidden], off[kDeepMaxHidden];
    const float *b[kDeepMaxHidden + 1];       // hidden biases, then the output bias [2D]
    const float *Wc[kDeepMaxHidden];           // Wc[0]: W1m transposed [D][U0]; Wc[l]: W_l m transposed [U_{l-1}][U_l]
    const float *Wo;                           // output masked weights [2D][U_{L-1}]
    const int *order, *ev_ptr, *ev;
    const float *aw;
};

__global__ void maf_masked_transpose_kernel(const float *__restrict__ W, const float *__restrict__ M, int rows, int cols,
                                            float *__restrict__ out) {
    const int64_t n = (int64_t)rows * cols;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / cols, c = e % cols;
        out[c * rows + r] = W[e] * M[e];
    }
}

__device__ __forceinline__ void deep_events(const DeepArgs &a, float *st, int lane, int slot) {
    const int e1 = a.ev_ptr[slot + 1];
    for (int e = a.ev_ptr[slot]; e < e1; ++e) {
        const int code = a.ev[e], l = code >> 16, j = code & 0xffff;
        float *hj = st + (a.off[l] + j) * 64 + lane;
        const float v = act_any(a.act, *hj);
        if (l + 1 == a.L) {
            *hj = v;
        } else {
            const float *w = a.Wc[l + 1] + (int64_t)j * a.U[l + 1];
            float *hn = st + a.off[l + 1] * 64 + lane;
            for (int k = 0; k < a.U[l + 1]; ++k) hn[k * 64] = fmaf(w[k], v, hn[k * 64]);
        }
    }
}

__global__ __launch_bounds__(64) void maf_sample_deep_kernel(DeepArgs a, const float *__restrict__ u, int64_t B,
                                                             float *__restrict__ x, float *__restrict__ ldj) {
    extern __shared__ float st[];              // [total units][64 lanes]: each lane touches its own column only
    const int lane = threadIdx.x, D = a.D;
    const int64_t b = (int64_t)blockIdx.x * 64 + lane;
    const bool live = b < B;
    const int64_t row = live ? b : 0;
    for (int l = 0; l < a.L; ++l)
        for (int j = 0; j < a.U[l]; ++j) st[(a.off[l] + j) * 64 + lane] = a.b[l][j];
    deep_events(a, st, lane, 0);
    const int UL = a.U[a.L - 1];
    const float *hL = st + a.off[a.L - 1] * 64 + lane;
    const float aw = a.aw[0];
    float acc = 0.f;
    for (int p = 0; p < D; ++p) {
        const int i = a.order[p];
        const float *wt = a.Wo + (int64_t)i * UL, *ws = a.Wo + (int64_t)(i + D) * UL;
        float t = a.b[a.L][i], sv = a.b[a.L][i + D];
        for (int k = 0; k < UL; ++k) {
            const float h = hL[k * 64];
            t = fmaf(wt[k], h, t);
            sv = fmaf(ws[k], h, sv);
        }
        const float sp = aw * tanhf(sv);
        const float xi = u[row * D + i] * expf(sp) + t;
        if (live) x[row * D + i] = xi;
        acc += sp;
        const float *w1 = a.Wc[0] + (int64_t)i * a.U[0];
        float *h1 = st + lane;
        for (int j = 0; j < a.U[0]; ++j) h1[j * 64] = fmaf(w1[j], xi, h1[j * 64]);
        deep_events(a, st, lane, p + 1);
    }
    if (live) ldj[b] = acc;
}

}  // namespace dpk

using namespace dpk;

// ---- C ABI -----------------------------------------------------------------------------------------------------------
extern "C" int64_t dpk_maf_chain_workspace_bytes(int64_t B, int32_t D, int32_t n_hidden, const int32_t *widths,
                                                 int32_t mode) {
    MafChain c;
    if (mode < 0 || mode > 2 || !chain_plan(B, D, n_hidden, widths, &c)) return DPK_EINVAL;
    return c.floats[mode] * 4 + 256;
}

extern "C" int dpk_maf_conditioner_forward(const float *x, int64_t B, int32_t D, int32_t n_hidden, const float *const *W,
                                           const float *const *M, const float *const *b, const int32_t *widths,
                                           int32_t activation, float *Z, void *ws, int64_t ws_bytes, void *stream) {
    MafChain c;
    int rc = chain_check("maf_conditioner_forward", x, B, D, n_hidden, W, M, b, widths, activation, &c);
    if (rc) return rc;
    DPK_REQUIRE(ws && (Z || B == 0), DPK_EINVAL, "maf_conditioner_forward: null pointer");
    if ((rc = chain_room("maf_conditioner_forward", c, 0, ws_bytes))) return rc;
    if (B == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    float *base = (float *)ws;
    DPK_TRY(chain_forward(c, base, x, B, D, W, M, b, activation, st, Z));
    return DPK_OK;
}

extern "C" int dpk_maf_density_chain(const float *x, int64_t B, int32_t D, int32_t n_hidden, const float *const *W,
                                     const float *const *M, const float *const *b, const int32_t *widths,
                                     int32_t activation, const float *act_weight, float *u, float *ildj, void *ws,
                                     int64_t ws_bytes, void *stream) {
    MafChain c;
    int rc = chain_check("maf_density_chain", x, B, D, n_hidden, W, M, b, widths, activation, &c);
    if (rc) return rc;
    DPK_REQUIRE(ws && act_weight && (B == 0 || (u && ildj)), DPK_EINVAL, "maf_density_chain: null pointer");
    if ((rc = chain_room("maf_density_chain", c, 1, ws_bytes))) return rc;
    if (B == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    float *base = (float *)ws;
    DPK_TRY(chain_forward(c, base, x, B, D, W, M, b, activation, st));
    DPK_LAUNCH("maf_epilogue_kernel", maf_epilogue_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, x,
               base + c.h_off[c.n_lin - 1], B, D, act_weight, u, ildj);
    return DPK_OK;
}

extern "C" int dpk_maf_density_chain_backward(const float *x, int64_t B, int32_t D, int32_t n_hidden,
                                              const float *const *W, const float *const *M, const float *const *b,
                                              const int32_t *widths, int32_t activation, const float *act_weight,
                                              const float *grad_u, const float *grad_ildj, const float *grad_Z,
                                              float *grad_x, float *const *grad_W, float *const *grad_b,
                                              float *grad_act, int32_t ws_holds_forward, void *ws, int64_t ws_bytes,
                                              void *stream) {
    MafChain c;
    int rc = chain_check("maf_density_chain_backward", x, B, D, n_hidden, W, M, b, widths, activation, &c);
    if (rc) return rc;
    DPK_REQUIRE(ws && grad_W && grad_b && (B == 0 || grad_x), DPK_EINVAL, "maf_density_chain_backward: null pointer");
    DPK_REQUIRE(grad_Z || act_weight, DPK_EINVAL, "maf_density_chain_backward: the epilogue needs the ScaledTanh weight");
    if ((rc = chain_room("maf_density_chain_backward", c, 2, ws_bytes))) return rc;
    hipStream_t st = (hipStream_t)stream;
    float *base = (float *)ws;
    if (B == 0) {
        int in = D;
        for (int l = 0; l < c.n_lin; ++l) {
            if (grad_W[l]) DPK_REQUIRE(hipMemsetAsync(grad_W[l], 0, (size_t)c.widths[l] * in * 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
            if (grad_b[l]) DPK_REQUIRE(hipMemsetAsync(grad_b[l], 0, (size_t)c.widths[l] * 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
            in = c.widths[l];
        }
        if (grad_act) DPK_REQUIRE(hipMemsetAsync(grad_act, 0, 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
        return DPK_OK;
    }
    if (!ws_holds_forward) DPK_TRY(chain_forward(c, base, x, B, D, W, M, b, activation, st));
    int64_t widest = 2 * (int64_t)D;
    for (int l = 0; l + 1 < c.n_lin; ++l) widest = c.widths[l] > widest ? c.widths[l] : widest;
    float *g0 = base + c.h_off[c.n_lin], *g1 = g0 + align_up(B * widest, 64), *pa = g1 + align_up(B * widest, 64);
    float *dOut = g0;
    if (grad_Z) {
        // gradient w.r.t. the conditioner output itself (the step loop's op): no epilogue, nothing direct into x
        DPK_REQUIRE(hipMemcpyAsync(dOut, grad_Z, (size_t)B * 2 * D * 4, hipMemcpyDeviceToDevice, st) == hipSuccess, DPK_ELAUNCH, "hipMemcpyAsync");
        DPK_REQUIRE(hipMemsetAsync(grad_x, 0, (size_t)B * D * 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
        if (grad_act) DPK_REQUIRE(hipMemsetAsync(grad_act, 0, 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
    } else {
        DPK_LAUNCH("maf_epilogue_bwd_kernel", maf_epilogue_bwd_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st, x,
                   base + c.h_off[c.n_lin - 1], B, D, act_weight, grad_u, grad_ildj, grad_x, dOut, pa);
        if (grad_act) DPK_LAUNCH("maf_colsum_kernel", maf_colsum_kernel, dim3(1), dim3(256), 0, st, pa, B, 1, grad_act,
            0);
    }
    for (int l = c.n_lin - 1; l >= 0; --l) {
        const int out_w = c.widths[l], in_w = l ? c.widths[l - 1] : D;
        const float *In = l ? base + c.h_off[l - 1] : x;
        if (grad_W[l]) {
            // dW = M * (dOut^T In)
            GemmArgs g{};
            g.A = dOut; g.sam = 1; g.sak = out_w;
            g.Bm = In; g.sbk = in_w; g.sbn = 1;
            g.C = grad_W[l]; g.ldc = in_w; g.M = out_w; g.N = in_w; g.K = (int)B;
            DPK_TRY(launch_gemm(g, st));
            const int64_t n = (int64_t)out_w * in_w;
            DPK_LAUNCH("maf_mul_kernel", maf_mul_kernel, dim3(grid_for(n)), dim3(256), 0, st, grad_W[l], M[l], n,
                       grad_W[l]);
        }
        if (grad_b[l]) DPK_LAUNCH("maf_colsum_kernel", maf_colsum_kernel, dim3(cdiv(out_w, 64)), dim3(256), 0, st, dOut,
            B, out_w, grad_b[l], 0);
        // dIn = dOut Wm (accumulated into grad_x for the first layer)
        float *dIn = l ? (dOut == g0 ? g1 : g0) : grad_x;
        GemmArgs g{};
        g.A = dOut; g.sam = out_w; g.sak = 1;
        g.Bm = base + c.wm_off[l]; g.sbk = in_w; g.sbn = 1;
        g.C = dIn; g.ldc = in_w; g.M = (int)B; g.N = in_w; g.K = out_w; g.accumulate = l == 0 ? 1 : 0;
        DPK_TRY(launch_gemm(g, st));
        if (l) {
            const int64_t n = B * in_w;
            DPK_LAUNCH("maf_act_bwd_kernel", maf_act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, st, dIn,
                       base + c.h_off[l - 1], n, activation);
        }
        dOut = dIn;
    }
    return DPK_OK;
}

extern "C" int64_t dpk_maf_density_workspace_bytes(int32_t D, int32_t units) {
    if (D < 2 || units < 1) return DPK_EINVAL;
    if (units > 256) return DPK_EUNSUPPORTED;
    return density_pack(D, units).floats * 4 + 256;
}

extern "C" int dpk_maf_density_forward(const float *x, int64_t B, int32_t D, const float *W1, const float *M1,
                                       const float *b1, const float *W2, const float *M2, const float *b2, int32_t units,
                                       int32_t activation, const float *act_weight, const float *in_scale,
                                       const float *in_shift, const int32_t *in_order, const int32_t *hidden_order,
                                       const int32_t *out_order, float *u, float *ildj, int32_t accumulate_ildj,
                                       void *ws, int64_t ws_bytes, void *stream) {
    DPK_REQUIRE(B >= 0 && D >= 2 && units >= 1 && activation >= 0 && activation <= 4, DPK_EINVAL,
                "maf_density_forward: bad sizes (B %lld, D %d, units %d, activation %d)", (long long)B, D, units, activation);
    DPK_REQUIRE(units <= 256, DPK_EUNSUPPORTED, "maf_density_forward: %d units (the fused kernel takes <= 256)", units);
    DPK_REQUIRE(W1 && M1 && b1 && W2 && M2 && b2 && act_weight && in_order && hidden_order && out_order && ws, DPK_EINVAL,
                "maf_density_forward: null pointer");
    DPK_REQUIRE(B == 0 || (x && u && ildj), DPK_EINVAL, "maf_density_forward: null pointer");
    const DensityPack p = density_pack(D, units);
    DPK_REQUIRE(ws_bytes >= p.floats * 4 + 256, DPK_EWORKSPACE, "maf_density_forward: workspace %lld < %lld",
                (long long)ws_bytes, (long long)(p.floats * 4 + 256));
    if (B == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    float *w = (float *)ws;
    const int64_t total = (int64_t)p.HT * 32 * p.KP + 2 * (int64_t)p.OT * 32 * p.UP + p.UP + 2 * p.OT * 32;
    DPK_LAUNCH("maf_pack_density_kernel", maf_pack_density_kernel, dim3(grid_for(total)), dim3(256), 0, st, p, W1, M1,
               b1, W2, M2, b2, in_order, hidden_order, out_order, w);
    DPK_LAUNCH("maf_klimit_kernel", maf_klimit_kernel, dim3(p.HT + p.OT), dim3(256), 0, st, p, M1, M2, in_order,
               hidden_order, out_order, w);
    const int nht = p.HT <= 4 ? 1 : 2;
    const int hs = p.UP + 1;
    const int lds = (64 * (hs > kFKc + 1 ? hs : kFKc + 1) + 256) * 4;
    dim3 grid(cdiv(B, kFRows));
    Profile prof(DPK_KERNEL_MAF_DENSITY, st);
    switch (activation) {
        case kActRelu: return launch_density<kActRelu>(prof, nht, p, grid, lds, st, x, B, w, in_order, out_order, act_weight, in_scale, in_shift, u, ildj, accumulate_ildj);
        case kActLeaky: return launch_density<kActLeaky>(prof, nht, p, grid, lds, st, x, B, w, in_order, out_order, act_weight, in_scale, in_shift, u, ildj, accumulate_ildj);
        case kActSoftplus: return launch_density<kActSoftplus>(prof, nht, p, grid, lds, st, x, B, w, in_order, out_order, act_weight, in_scale, in_shift, u, ildj, accumulate_ildj);
        case kActTanh: return launch_density<kActTanh>(prof, nht, p, grid, lds, st, x, B, w, in_order, out_order, act_weight, in_scale, in_shift, u, ildj, accumulate_ildj);
        default: return launch_density<kActSigmoid>(prof, nht, p, grid, lds, st, x, B, w, in_order, out_order, act_weight, in_scale, in_shift, u, ildj, accumulate_ildj);
    }
}

extern "C" int64_t dpk_maf_sample_workspace_bytes(int32_t D, int32_t units) {
    if (D < 1 || units < 1) return DPK_EINVAL;
    if (units > 128) return DPK_EUNSUPPORTED;
    return sample_pack(D, units).floats * 4 + 256;
}

extern "C" int dpk_maf_sample_forward(const float *u, int64_t B, int32_t D, const float *W1, const float *M1,
                                      const float *b1, const float *W2, const float *M2, const float *b2, int32_t units,
                                      int32_t activation, const float *act_weight, const int32_t *order, float *x,
                                      float *ldj, void *ws, int64_t ws_bytes, void *stream) {
    DPK_REQUIRE(B >= 0 && D >= 1 && units >= 1 && activation >= 0 && activation <= 4, DPK_EINVAL,
                "maf_sample_forward: bad sizes (B %lld, D %d, units %d, activation %d)", (long long)B, D, units, activation);
    DPK_REQUIRE(units <= 128, DPK_EUNSUPPORTED, "maf_sample_forward: %d units (the sampling kernel takes <= 128)", units);
    DPK_REQUIRE(W1 && M1 && b1 && W2 && M2 && b2 && act_weight && order && ws, DPK_EINVAL, "maf_sample_forward: null pointer");
    DPK_REQUIRE(B == 0 || (u && x && ldj), DPK_EINVAL, "maf_sample_forward: null pointer");
    const SamplePack p = sample_pack(D, units);
    DPK_REQUIRE(ws_bytes >= p.floats * 4 + 256, DPK_EWORKSPACE, "maf_sample_forward: workspace %lld < %lld",
                (long long)ws_bytes, (long long)(p.floats * 4 + 256));
    if (B == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    float *w = (float *)ws;
    const int64_t total = (int64_t)D * 3 * p.UP + 2 * (int64_t)D + p.UP;
    DPK_LAUNCH("maf_pack_sample_kernel", maf_pack_sample_kernel, dim3(grid_for(total)), dim3(256), 0, st, p, W1, M1, b1,
               W2, M2, b2, order, w);
    DPK_LAUNCH("maf_sample_nz_kernel", maf_sample_nz_kernel, dim3(cdiv(D, 4)), dim3(256), 0, st, p, w);
    dim3 grid(cdiv(B, kSThreads));
    Profile prof(DPK_KERNEL_MAF_SAMPLE, st);
    switch (activation) {
        case kActRelu: return launch_sample<kActRelu>(prof, p.UP, grid, st, p, u, B, w, order, act_weight, x, ldj);
        case kActLeaky: return launch_sample<kActLeaky>(prof, p.UP, grid, st, p, u, B, w, order, act_weight, x, ldj);
        case kActSoftplus: return launch_sample<kActSoftplus>(prof, p.UP, grid, st, p, u, B, w, order, act_weight, x, ldj);
        case kActTanh: return launch_sample<kActTanh>(prof, p.UP, grid, st, p, u, B, w, order, act_weight, x, ldj);
        default: return launch_sample<kActSigmoid>(prof, p.UP, grid, st, p, u, B, w, order, act_weight, x, ldj);
    }
}

extern "C" int64_t dpk_masked_linear_workspace_bytes(int32_t in_features, int32_t out_features) {
    if (in_features < 1 || out_features < 1) return DPK_EINVAL;
    return align_up((int64_t)in_features * out_features * 4, 256) + 256;
}

extern "C" int dpk_masked_linear_forward(const float *x, int64_t B, int32_t in_features, int32_t out_features,
                                         const float *W, const float *M, const float *b, float *y, void *ws,
                                         int64_t ws_bytes, void *stream) {
    DPK_REQUIRE(B >= 0 && in_features >= 1 && out_features >= 1, DPK_EINVAL, "masked_linear_forward: bad sizes");
    DPK_REQUIRE(W && M && ws && (B == 0 || (x && y)), DPK_EINVAL, "masked_linear_forward: null pointer");
    const int64_t need = dpk_masked_linear_workspace_bytes(in_features, out_features);
    DPK_REQUIRE(ws_bytes >= need, DPK_EWORKSPACE, "masked_linear_forward: workspace %lld < %lld", (long long)ws_bytes,
                (long long)need);
    if (B == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)in_features * out_features;
    DPK_LAUNCH("maf_mul_kernel", maf_mul_kernel, dim3(grid_for(n)), dim3(256), 0, st, W, M, n, (float *)ws);
    GemmArgs g{};
    g.A = x; g.sam = in_features; g.sak = 1;
    g.Bm = (const float *)ws; g.sbk = 1; g.sbn = in_features;
    g.C = y; g.ldc = out_features; g.M = (int)B; g.N = out_features; g.K = in_features; g.bias = b;
    DPK_TRY(launch_gemm(g, st));
    return DPK_OK;
}

extern "C" int dpk_masked_linear_backward(const float *x, int64_t B, int32_t in_features, int32_t out_features,
                                          const float *W, const float *M, const float *grad_y, float *grad_x,
                                          float *grad_W, float *grad_b, void *ws, int64_t ws_bytes, void *stream) {
    DPK_REQUIRE(B >= 0 && in_features >= 1 && out_features >= 1, DPK_EINVAL, "masked_linear_backward: bad sizes");
    DPK_REQUIRE(W && M && ws && (B == 0 || (x && grad_y)), DPK_EINVAL, "masked_linear_backward: null pointer");
    const int64_t need = dpk_masked_linear_workspace_bytes(in_features, out_features);
    DPK_REQUIRE(ws_bytes >= need, DPK_EWORKSPACE, "masked_linear_backward: workspace %lld < %lld", (long long)ws_bytes,
                (long long)need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)in_features * out_features;
    if (B == 0) {
        if (grad_W) DPK_REQUIRE(hipMemsetAsync(grad_W, 0, (size_t)n * 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
        if (grad_b) DPK_REQUIRE(hipMemsetAsync(grad_b, 0, (size_t)out_features * 4, st) == hipSuccess, DPK_ELAUNCH, "hipMemsetAsync");
        return DPK_OK;
    }
    if (grad_x) {
        DPK_LAUNCH("maf_mul_kernel", maf_mul_kernel, dim3(grid_for(n)), dim3(256), 0, st, W, M, n, (float *)ws);
        GemmArgs g{};
        g.A = grad_y; g.sam = out_features; g.sak = 1;
        g.Bm = (const float *)ws; g.sbk = in_features; g.sbn = 1;
        g.C = grad_x; g.ldc = in_features; g.M = (int)B; g.N = in_features; g.K = out_features;
        DPK_TRY(launch_gemm(g, st));
    }
    if (grad_W) {
        GemmArgs g{};
        g.A = grad_y; g.sam = 1; g.sak = out_features;
        g.Bm = x; g.sbk = in_features; g.sbn = 1;
        g.C = grad_W; g.ldc = in_features; g.M = out_features; g.N = in_features; g.K = (int)B;
        DPK_TRY(launch_gemm(g, st));
        DPK_LAUNCH("maf_mul_kernel", maf_mul_kernel, dim3(grid_for(n)), dim3(256), 0, st, grad_W, M, n, grad_W);
    }
    if (grad_b) DPK_LAUNCH("maf_colsum_kernel", maf_colsum_kernel, dim3(cdiv(out_features, 64)), dim3(256), 0, st,
        grad_y, B, out_features, grad_b, 0);
    return DPK_OK;
}

extern "C" int64_t dpk_maf_sample_deep_workspace_bytes(int32_t D, int32_t n_hidden, const int32_t *widths) {
    if (D < 1 || n_hidden < 2 || !widths) return DPK_EINVAL;
    if (n_hidden > kDeepMaxHidden) return DPK_EUNSUPPORTED;
    int64_t total = 0, floats = 0, in = D;
    for (int l = 0; l < n_hidden; ++l) {
        if (widths[l] < 1) return DPK_EINVAL;
        total += widths[l];
        floats += align_up(in * widths[l], 64);
        in = widths[l];
    }
    if (total > kDeepMaxUnits) return DPK_EUNSUPPORTED;
    floats += align_up(2 * (int64_t)D * in, 64);
    return floats * 4 + 256;
}

extern "C" int dpk_maf_sample_deep_forward(const float *u, int64_t B, int32_t D, int32_t n_hidden, const float *const *W,
                                           const float *const *M, const float *const *b, const int32_t *widths,
                                           int32_t activation, const float *act_weight, const int32_t *order,
                                           const int32_t *event_ptr, const int32_t *events, float *x, float *ldj,
                                           void *ws, int64_t ws_bytes, void *stream) {
    DPK_REQUIRE(B >= 0 && D >= 1 && n_hidden >= 2 && activation >= 0 && activation <= 4 && widths, DPK_EINVAL,
                "maf_sample_deep_forward: bad sizes (B %lld, D %d, n_hidden %d, activation %d)", (long long)B, D, n_hidden,
                activation);
    const int64_t need = dpk_maf_sample_deep_workspace_bytes(D, n_hidden, widths);
    if (need < 0) {
        DPK_REQUIRE(need != DPK_EUNSUPPORTED, DPK_EUNSUPPORTED, "maf_sample_deep_forward: outside the envelope (<= %d hidden "
                    "layers, <= %d hidden units in all)", kDeepMaxHidden, kDeepMaxUnits);
        DPK_REQUIRE(false, DPK_EINVAL, "maf_sample_deep_forward: bad widths");
    }
    DPK_REQUIRE(W && M && b && act_weight && order && event_ptr && events && ws, DPK_EINVAL,
                "maf_sample_deep_forward: null pointer");
    for (int l = 0; l <= n_hidden; ++l)
        DPK_REQUIRE(W[l] && M[l] && b[l], DPK_EINVAL, "maf_sample_deep_forward: null parameter %d", l);
    DPK_REQUIRE(B == 0 || (u && x && ldj), DPK_EINVAL, "maf_sample_deep_forward: null pointer");
    DPK_REQUIRE(ws_bytes >= need, DPK_EWORKSPACE, "maf_sample_deep_forward: workspace %lld < %lld", (long long)ws_bytes,
                (long long)need);
    if (B == 0) return DPK_OK;
    hipStream_t st = (hipStream_t)stream;
    DeepArgs a{};
    a.D = D; a.L = n_hidden; a.act = activation;
    float *w = (float *)ws;
    int64_t o = 0, in = D;
    for (int l = 0; l < n_hidden; ++l) {
        a.U[l] = widths[l];
        a.off[l] = a.total;
        a.total += widths[l];
        a.b[l] = b[l];
        DPK_LAUNCH("maf_masked_transpose_kernel", maf_masked_transpose_kernel, dim3(grid_for(in * widths[l])),
                   dim3(256), 0, st, W[l], M[l], widths[l], (int)in, w + o);
        a.Wc[l] = w + o;
        o += align_up(in * widths[l], 64);
        in = widths[l];
    }
    a.b[n_hidden] = b[n_hidden];
    DPK_LAUNCH("maf_mul_kernel", maf_mul_kernel, dim3(grid_for(2 * (int64_t)D * in)), dim3(256), 0, st, W[n_hidden],
               M[n_hidden], 2 * (int64_t)D * in, w + o);
    a.Wo = w + o;
    a.order = order; a.ev_ptr = event_ptr; a.ev = events; a.aw = act_weight;
    const int lds = a.total * 64 * 4;
    DPK_TRY(ensure_dynamic_lds((const void *)maf_sample_deep_kernel, lds));
    Profile prof(DPK_KERNEL_MAF_SAMPLE, st);
    DPK_LAUNCH_IN(prof, "maf_sample_deep_kernel", maf_sample_deep_kernel, dim3(cdiv(B, 64)), dim3(64), lds, st, a, u, B,
                  x, ldj);
    return DPK_OK;
}
