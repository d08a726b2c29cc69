/*
 * monorun_targets.h — C ABI of the NOC head's LiDAR supervision in libmonorun_pnp.so: the dense NOC targets and loss_noc.  The entry
 * points are compiled into the same library as those of monorun_pnp.h and follow its conventions: 0 on success or a negative MR_ERR_*
 * code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernel, in stream order; a call runs on the
 * current HIP device, asynchronously on `stream`; nothing is allocated.  The per-image tables of mr_noc_dense_target are HOST arrays
 * (of device pointers, sizes and flags), read during the call as the per-call tables of the grouped entry points are.
 *
 * Reference interface replaced: MonoRUnRoIHead._noc_forward_train of the MonoRUn tree (monorun/models/roi_heads/monorun_roi_head.py:343-365):
 * NOCCoder.encode (core/bbox_3d/coord_coder/noc_coder.py:17-48), masked_dense_target (core/bbox_3d/masked_dense_target.py) and
 * SmoothL1LossMod (models/losses/smooth_l1_loss.py).
 */
#ifndef MONORUN_TARGETS_H_
#define MONORUN_TARGETS_H_

#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_NOC_TARGET_MAX_IMAGES 32

/*
 * The dense NOC targets of n positive RoIs in num_images images, TWO launches (no memset, no host synchronisation, no copy of a map).
 * Image j has G_j = num_gt[j] ground truths with maps of map_h[j] x map_w[j] pixels: coords_3d[j] (G_j, 3, H_j, W_j) the masked
 * coordinates, coords_3d_mask[j] (G_j, 1, H_j, W_j) the mask, both fp32 contiguous; dimensions[j] rows of at least 3 fp32 [l, h, w, ...]
 * dimensions_row_stride[j] elements apart; flip[j] nonzero for a flipped image.  RoI i: rois (n, 4) fp32 [x1, y1, x2, y2] in its image's
 * pixels, roi_img (n) int32 its image, roi_gt (n) int64 its ground truth in that image.  target_means, target_stds (3) fp32.
 *
 * Per pixel of ground truth g (the coder's encode, fp32, every operation a separate IEEE operation in this order):
 *   fg = m >= eps_coder;  part_k = c_k / max(m, eps_coder) / max(dim_k, eps_coder);  part_2 = -part_2 in a flipped image;
 *   m' = fg ? m : 0;      enc_k = ((part_k - mean_k) / std_k) m'
 * Per RoI: x clipped to [0, W_j], y to [0, H_j]; T = roi_align(enc[g], roi, (h, w), 1.0, 0, 'avg', True), M = roi_align(m'[g], ...)
 * (mr_roi_align_avg's arithmetic; the encode is applied to the four corner pixels of each bilinear tap, which is the same numbers);
 * wgt = M > eps_target;  T = wgt ? T / M : T.  Then weights = wgt / max(fp32(sum wgt) / fp32(n h w), eps_target), the sum an integer.
 *
 * Outputs (device, contiguous, EVERY element written): targets (n, 3, h, w) fp32, weights (n, 1, h, w) fp32, counts (n) int32 — the
 * number of bins with wgt of each RoI (scratch of the second launch, valid afterwards).
 *
 * The one deviation from the reference, which would index out of range: a RoI with roi_img outside [0, num_images), roi_gt outside
 * [0, G_j) or a clipped coordinate that is not finite (NaN) reads no map and gets zero targets, zero weights and count 0; the call
 * still returns 0.  The tap counts of any other RoI are bounded by H_j and W_j.
 *
 * n = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for n < 0, num_images < 0, h < 1, w < 1, a NULL required pointer or table,
 * map_h / map_w < 1, num_gt < 0, a NULL map or dimensions pointer of an image with num_gt > 0 or a row stride below 3;
 * MR_ERR_UNSUPPORTED for num_images > MR_NOC_TARGET_MAX_IMAGES or n h w > 2^31 - 1.
 */
int mr_noc_dense_target(int num_images, const float *const *coords_3d, const float *const *coords_3d_mask, const float *const *dimensions,
                        const int64_t *dimensions_row_stride, const int32_t *map_h, const int32_t *map_w, const int32_t *num_gt,
                        const uint8_t *flip, const float *rois, const int32_t *roi_img, const int64_t *roi_gt, int n, int h, int w,
                        const float *target_means, const float *target_stds, double eps_coder, double eps_target,
                        float *targets, float *weights, int32_t *counts, void *stream);

/* Bytes of workspace mr_smooth_l1_mod_loss needs for numel elements (a multiple of 256; 0 for numel <= 0). */
int64_t mr_smooth_l1_mod_workspace_bytes(int64_t numel);

/*
 * SmoothL1LossMod, reduced, two launches: per element l = d < beta ? 0.5 d d / beta : d - (float)(0.5 beta) with d = |pred - target|, times
 * the element weight, in fp32; the sum in fp64 (per thread, per workgroup to the workspace, then one workgroup in a fixed order: no atomics,
 * bitwise reproducible); loss[0] = (float)loss_weight * (float)(reduction == 0 ? sum / numel : sum).
 * pred, target (numel) fp32; weight NULL (weight_mode 0), (numel) (1) or, for pred of shape (n, channels, hw), (n, 1, hw) broadcast over the
 * channels (2).  reduction 0 'mean', 1 'sum'.
 * MR_ERR_BAD_ARGUMENT for numel < 1, beta <= 0, another reduction or weight_mode, a NULL pointer (weight with mode 1 or 2), channels or hw < 1
 * or numel no multiple of channels * hw in mode 2, a workspace smaller than mr_smooth_l1_mod_workspace_bytes(numel).
 */
int mr_smooth_l1_mod_loss(const float *pred, const float *target, const float *weight, int weight_mode, int64_t numel, int channels, int64_t hw,
                          double beta, int reduction, double loss_weight, float *loss, void *workspace, int64_t workspace_bytes, void *stream);

/*
 * Its gradient to pred, ONE launch: with g = grad_loss[0] (float)loss_weight [/ (float)numel] [weight],
 * grad_pred = sgn(pred - target) (d < beta ? g d / beta : g), 0 where pred == target.  target and weight get no gradient.
 * Errors as mr_smooth_l1_mod_loss; MR_ERR_UNSUPPORTED for more than 2^31 - 1 workgroups.
 */
int mr_smooth_l1_mod_loss_backward(const float *pred, const float *target, const float *weight, int weight_mode, int64_t numel, int channels,
                                   int64_t hw, double beta, int reduction, double loss_weight, const float *grad_loss, float *grad_pred,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif
