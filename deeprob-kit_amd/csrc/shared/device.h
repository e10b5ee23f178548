// Device primitives that the samplers and top-down passes of every library share: counter_uniform (the draw), wave_max_nan
// and wave_sum, block_max_nan<WAVES> and block_sum<WAVES> (the same over a work-group; the moment kernels of rat/ and dgc/),
// wave_inverse_cdf.  Header-only and force-inlined: each includer compiles them under its own flags (the small libraries
// with -ffp-contract=off, libdeeprob_hip.so without).  The node functions of a flattened SPN are in flat_spn_nodes.h.
//
// The draw.  Every sampler of the project is counter based, so that a test can replay it from Python:
//
//     u(seed, ctr) = (splitmix64(seed + ctr * 0x9E3779B97F4A7C15) >> 40) / 2^24          (a float in [0, 1), 24 bits)
//     splitmix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
//
// in 64-bit wrapping arithmetic.  The tests restate exactly this (tests/*_ref.py); the formula never changes.  What `ctr`
// means -- the layout of a row's slots -- is the includer's and is documented there.
#pragma once
#include <hip/hip_runtime.h>

namespace dp_device {

__device__ __forceinline__ float counter_uniform(unsigned long long seed, unsigned long long ctr) {
    unsigned long long z = seed + ctr * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(unsigned)(z >> 40) * (1.0f / 16777216.0f);
}

// NaN-propagating maximum over the wave (an impossible or undefined node must be seen, not skipped)
__device__ __forceinline__ float wave_max_nan(float m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(m, o, 64);
        m = (t > m || t != t) ? t : m;
    }
    return m;
}

// (a butterfly: every lane ends with the same bits)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The same over a work-group of WAVES waves, through red[WAVES] in LDS: the waves' results are combined in wave order by
// every thread, so all end with the same bits.  Every thread of the work-group calls; red is free again on return.
template <int WAVES>
__device__ __forceinline__ float block_max_nan(float m, float *red) {
    m = wave_max_nan(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
        const float t = red[w];
        m = (t > m || t != t) ? t : m;
    }
    __syncthreads();
    return m;
}

template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += red[w];
    __syncthreads();
    return v;
}

// inverse CDF in index order over the non-negative weight(n), by a wave: lane l owns the contiguous chunk [l ch, (l + 1) ch),
// sums it in order, the chunks are scanned over the lanes; target = u * total, the first n with target < c(n), the last
// input when rounding leaves none.  Every lane returns the pick.
template <typename WeightFn>
__device__ __forceinline__ int wave_inverse_cdf(int count, int lane, float u, WeightFn weight) {
    const int ch = (count + 63) / 64;
    const int n0 = min(lane * ch, count), n1 = min(n0 + ch, count);
    float s = 0.f;
    for (int n = n0; n < n1; ++n) s += weight(n);
    float inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    const float total = __shfl(inc, 63, 64);
    const float target = u * total;
    const unsigned long long hit = __ballot(target < inc && n1 > n0);
    int pick = count - 1;                          // (target >= total by rounding: the last input)
    if (hit != 0ull) {
        const int owner = __ffsll((long long)hit) - 1;
        int mine = n1 - 1;
        if (lane == owner) {
            float c = inc - s;
            for (int n = n0; n < n1; ++n) {
                c += weight(n);
                if (target < c) {
                    mine = n;
                    break;
                }
            }
        }
        pick = __shfl(mine, owner, 64);
    }
    return pick;
}

}  // namespace dp_device
