// The generic fp32-MFMA GEMM of the training routes (defined in coupling_bwd.hip): C = epilogue(A B), operands
// addressed through strides so that transposed products need no copies.  Shared by the RealNVP-1D training route and
// the MAF conditioner (maf.hip).
#pragma once
#include "common.h"

namespace dpk {

struct GemmArgs {
    const float *A, *Bm;
    float *C;
    int M, N, K;
    int64_t sam, sak, sbk, sbn, ldc;
    const float *kscale;   // A(m,k) *= kscale[k]
    const float *nscale;   // result(m,n) *= nscale[n]
    const float *bias;     // + bias[n] (before relu)
    const float *gate;     // result zeroed where gate[m*ldg + n] <= 0
    int64_t ldg;
    int relu, accumulate;
    int ksplit, kchunk;    // > 1: blockIdx.z owns K range [z*kchunk, (z+1)*kchunk)
    float *partials;       // split-K: [tile][slice][16][256] partial tiles; the last slice to finish a tile sums them in slice
    unsigned *tickets;     // order and runs the epilogue ([tile] arrival counts, zero between launches).  Null: the partial
};                         // sums meet by atomicAdd into a zeroed C and gemm_epilogue_kernel follows (fallback)

// One product on `st`: K split over blockIdx.z (partial tiles summed in slice order) when the output tiles alone do not
// fill the chip.  M <= 0 or N <= 0 launches nothing.
int launch_gemm(const GemmArgs &g, hipStream_t st);

}  // namespace dpk
