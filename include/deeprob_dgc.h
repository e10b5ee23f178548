/*
 * deeprob_dgc.h -- C ABI of libdeeprob_dgc.so (gfx950 / MI355X): the top-down pass of a DGC-SPN
 * (deeprob.spn.models.DgcSpn.sample / sample_conditional / mpe_completion) in one launch.
 *
 * The reference raises in DgcSpn.sample (deeprob/spn/models/dgcspn.py) and has no conditional
 * sampler.  The pass is defined, statement for statement, at the top of
 * deeprob-kit_amd/csrc/dgc/dgcspn_topdown.hip; this header states the tables it takes.
 *
 * The model: L product levels j = 0 .. L-1 (2x2 windows, SpatialProductLayer) with a SpatialSumLayer
 * t = j + 1 on top of every level but the last, Gaussian leaves below level 0, a root over the
 * flattened output of level L-1.
 *
 * geom: [L][DPG_GEOM_INTS] int32 in HOST memory, one row per product level:
 *   Cin, Hin, Win, Cout, Hout, Wout, pad_left, pad_right, pad_top, pad_bottom, stride, dilation,
 *   depthwise (0 / 1).
 * The input coordinate of tap (th, tw) of output (oh, ow) is (oh * stride + th * dilation - pad_top,
 * ow * stride + tw * dilation - pad_left); a tap outside [0, Hin) x [0, Win) is the constant log 1.
 * A depthwise level has Cout = Cin and every tap reads channel oc; any other level has
 * Cout = Cin^4 and tap t = 2 th + tw reads channel (oc / Cin^(3-t)) % Cin (itertools.product
 * order).  Level 0 reads the leaf map (Cin = K, Hin = H, Win = W); level j > 0 reads the output of
 * sum layer j, [Cin_j, Hin_j, Win_j] with (Hin_j, Win_j) = (Hout_{j-1}, Wout_{j-1}).  Every map has
 * at most 65535 positions and at most 32767 channels; stride, dilation and the pads are at most 65535
 * in magnitude; at most 4096 positions of one map can be active (an image of up to 64 x 64 pixels).
 *
 * act:  [L] pointers in HOST memory to DEVICE maps, fp32 NCHW: act[0] the leaf layer's output
 *       [B, K, H, W], act[t] the output of sum layer t [B, Cin_t, Hin_t, Win_t].  NULL in mode 1.
 * logw: [L + 1] pointers in HOST memory to DEVICE tables: logw[t], 1 <= t < L, the
 *       log_softmax(weight, 1) of sum layer t, [Cin_t, Cout_{t-1}, Hout_{t-1}, Wout_{t-1}];
 *       logw[L] the root's, [classes, Cout_{L-1} * Hout_{L-1} * Wout_{L-1}].  logw[0] is not read.
 *
 * Counter layout of the draws: u(ctr) = (splitmix64(seed + ctr * 0x9E3779B97F4A7C15) >> 40) / 2^24
 * (the generator of dpk_ratspn_topdown) with ctr = row * slots_per_row + slot,
 *   slot 0                                    the root's draw,
 *   slot base_t + h * Wout_{t-1} + w          the draw of sum layer t at position (h, w), with
 *                                             base_1 = 1, base_{t+1} = base_t + Hout_{t-1} * Wout_{t-1},
 *   slot base_L + 2 * ((c * H + h) * W + w), + 1   the two uniforms of leaf entry (c, h, w),
 *   slots_per_row = base_L + 2 * C * H * W.
 *
 * Every other pointer is a DEVICE pointer; `stream` is a hipStream_t passed as void*; the kernel is
 * enqueued asynchronously on it and the entry point neither synchronises nor allocates.
 *
 * Buffer contract (the one of include/deeprob_hip.h, repeated):
 *   1. an entry point writes only its output arguments, over their documented extent;
 *   2. it writes every element of every output, for every legal shape (B = 0 writes nothing);
 *   3. nothing it does depends on what the outputs held on entry;
 *   4. it leaves its `const` inputs alone.
 * There is no workspace, no floating-point value is accumulated atomically, and no kernel waits on
 * another work-group.
 *
 * The return value is 0 on success and a negative DPG_E* code otherwise; dpg_last_error() returns
 * a thread-local message for the last failure.
 */
#ifndef DEEPROB_DGC_H
#define DEEPROB_DGC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPG_OK 0
#define DPG_EINVAL (-1)  /* bad argument (null pointer, size out of domain, inconsistent geometry) */
#define DPG_ELAUNCH (-3) /* hipLaunch / runtime error                                             */

#define DPG_GEOM_INTS 13    /* int32 per row of `geom`                                             */
#define DPG_MAX_LEVELS 12   /* most product levels: ceil(log2(H)) + 1                              */
#define DPG_MODE_PRIOR 1     /* every activation is log 1: the weights alone, `act` and `x` unused  */
#define DPG_MODE_POSTERIOR 2 /* scores from the activations of a bottom-up pass under `x`           */
#define DPG_MODE_MPE 3       /* mode 2's scores, selected from where mode 2 draws: max-product       */

const char *dpg_last_error(void);
int dpg_abi_version(void);

/* One draw per row from p(x | y) (mode 1) or p(x_missing | x_observed, y) (mode 2).
 * x: [B, C, H, W] evidence, NaN = to be drawn; NULL: everything is drawn (always so in mode 1).
 * y: [B] int64 class of the root to descend from (clamped to [0, classes)); NULL: class 0.
 * loc, scale: [K, C, H, W] leaf parameters.
 * out: [B, C, H, W].  An observed entry is x bit for bit, a NaN entry of a pixel in scope is
 *      loc + scale * z of the component drawn for the pixel, and a pixel that no path from the root
 *      reaches (dropped by a 'valid' stride-2 level of an odd map) is returned as given: its evidence,
 *      or NaN.
 * choice: optional [B, 1 + H * W] int32: the root's input index, then per pixel the leaf component
 *      drawn, -1 for a pixel out of scope.
 * A row's output depends on (seed, row index, y[row]) and the row's evidence only.
 *
 * Mode 3 (DPG_MODE_MPE) takes the arguments of mode 2 (x may be NULL, act is required) and selects
 * where mode 2 draws; `seed` is ignored and no uniform is formed.  At the root and at every active
 * position of every sum layer, with mode 2's fp32 scores s(n) = prod_value(n) + logw(n),
 * prod_value = ((v0 + v1) + v2) + v3, and their NaN-sticky maximum m: if m > -inf the first n in index
 * order with s(n) == m; otherwise (m is -inf or NaN) the first n in index order that maximises
 * logw(n), a NaN weight never over a number.  Ties always go to the lowest index.  A NaN entry of a
 * pixel reached with component k is loc[k, c, h, w] bit for bit (the mode of a Gaussian; `scale` is
 * not read); observed entries, pixels out of scope and `choice` are as in mode 2.  The result is the
 * leaf modes of the induced tree chosen greedily from the sum-pass activations -- not a global MAP.
 * A row's output depends on y[row] and the row's evidence only. */
int dpg_dgcspn_topdown(int32_t mode, int64_t B, int32_t C, int32_t H, int32_t W, int32_t K, int32_t n_levels,
                       const int32_t *geom, int32_t classes, const float *x, const int64_t *y,
                       const float *const *act, const float *const *logw, const float *loc, const float *scale,
                       uint64_t seed, float *out, int32_t *choice, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_DGC_H */
