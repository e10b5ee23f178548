/*
 * deeprob_dgcm.h -- exact posterior moments of the missing entries of a DGC-SPN
 * (deeprob.spn.models.DgcSpn.posterior_moments / expectation / variance) in one launch, exported by
 * libdeeprob_dgc.so beside the entry points of deeprob_dgc.h (prefix dpm_: that header's list stays
 * what it is).
 *
 * The reference offers DgcSpn.mpe only (deeprob/spn/models/dgcspn.py: autograd through every layer,
 * means without variances).  The pass is defined, statement for statement, at the top of
 * deeprob-kit_amd/csrc/dgc/dgcspn_moments.hip: the posterior flow of every sum node goes to ALL of its
 * inputs, top to bottom, and the leaf components of a pixel are mixed by the flow they receive.
 *
 * The model, the geometry table `geom` ([L][DPG_GEOM_INTS] int32 in HOST memory) with its limits, and
 * the tables `act` ([L] pointers in HOST memory to DEVICE maps) and `logw` ([L + 1] pointers in HOST
 * memory to DEVICE tables, logw[0] not read) are those of include/deeprob_dgc.h, mode 2.
 *
 * Workspace.  The flow maps of one image do not fit on chip at the sizes that matter, so every
 * work-group owns a slice of a caller-supplied DEVICE workspace: |F| + |G| floats,
 *   |F| = max_j Cin_j Hin_j Win_j    (the flow into the leaf map and into every sum layer's map),
 *   |G| = max_j Cout_j Hout_j Wout_j (the flow into every product map),
 * and the launch has min(B, DPM_MAX_GROUPS) work-groups that walk the batch grid-stride:
 *   dpm_dgcspn_moments_workspace_bytes = min(B, DPM_MAX_GROUPS) * (|F| + |G|) * 4.
 * A slice is written and read by its own work-group only.
 *
 * Every other pointer is a DEVICE pointer; `stream` is a hipStream_t passed as void*; the kernel is
 * enqueued asynchronously on it and the entry point neither synchronises nor allocates.
 *
 * Buffer contract (the one of include/deeprob_hip.h, repeated):
 *   1. an entry point writes only its output arguments and its workspace, over their documented extent;
 *   2. it writes every element of every output, for every legal shape (B = 0 writes nothing);
 *   3. nothing it does depends on what the outputs or the workspace held on entry;
 *   4. it leaves its `const` inputs alone.
 * No floating-point value is accumulated atomically and no kernel waits on another work-group: every
 * sum has an order that depends on the shape only, so a row's output depends on the row and the model
 * only, whatever the batch and the grid, and two calls give the same bits.
 *
 * The return value is 0 on success (a size for *_workspace_bytes) and a negative DPM_E* code
 * otherwise; dpm_last_error() returns the library's thread-local message for the last failure (the
 * text dpg_last_error() returns: one library, one text).
 */
#ifndef DEEPROB_DGCM_H
#define DEEPROB_DGCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPM_OK 0
#define DPM_EINVAL (-1)     /* bad argument (null pointer, size out of domain, inconsistent geometry) */
#define DPM_EWORKSPACE (-2) /* workspace too small                                                    */
#define DPM_ELAUNCH (-3)    /* hipLaunch / runtime error                                              */

#define DPM_MAX_GROUPS 768 /* most work-groups of a launch = most workspace slices */

const char *dpm_last_error(void);

/* Bytes of workspace dpm_dgcspn_moments needs for B images of this geometry (0 for B = 0). */
int64_t dpm_dgcspn_moments_workspace_bytes(int64_t B, int32_t n_levels, const int32_t *geom);

/* Posterior mean and variance of every NaN entry of x given the image's observed entries.
 * x: [B, C, H, W] evidence, NaN = missing.
 * y: [B] int64 class of the root to descend from (clamped to [0, classes)); NULL: class 0, or with
 *    all_classes != 0 the mixture of the classes under the uniform class prior.
 * act, logw: the bottom-up activations under x and the log-softmax weights (deeprob_dgc.h).
 * loc, scale: [K, C, H, W] leaf parameters.
 * mean: [B, C, H, W].  An observed entry is x bit for bit; a NaN entry of a pixel in scope is
 *      E[x | e, y]; a NaN entry of a pixel that no path from the root reaches stays NaN.
 * var: optional [B, C, H, W]: 0 / Var[x | e, y] / NaN in the same three cases.
 * leaf_flow: optional [B, K, H, W] = d log p(e, y) / d act[0]: the posterior probability that pixel
 *      (h, w) is reached with component k (0 at a pixel out of scope).
 * An image whose root maximum is -inf or NaN (evidence impossible under the model) has NaN in the
 * NaN entries of mean and var, its observed entries as given, and NaN in leaf_flow.
 * workspace: at least dpm_dgcspn_moments_workspace_bytes(B, n_levels, geom) bytes, 4-byte aligned. */
int dpm_dgcspn_moments(int64_t B, int32_t C, int32_t H, int32_t W, int32_t K, int32_t n_levels, const int32_t *geom,
                       int32_t classes, int32_t all_classes, const float *x, const int64_t *y,
                       const float *const *act, const float *const *logw, const float *loc, const float *scale,
                       float *mean, float *var, float *leaf_flow, void *workspace, int64_t workspace_bytes,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPROB_DGCM_H */
