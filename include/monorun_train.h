/*
 * monorun_train.h — C ABI of the training kernels of libmonorun_pnp.so that sit between the NOC head and its losses.  The entry points
 * are compiled into the same library as those of monorun_pnp.h and follow its conventions: 0 on success or a negative MR_ERR_* code
 * of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernel, in stream order; a call runs on the
 * current HIP device, asynchronously on `stream`; nothing is allocated.
 *
 * Reference interface replaced: the training decode chain of MonoRUnRoIHead.forward_train of the MonoRUn tree
 * (monorun/models/roi_heads/monorun_roi_head.py:189-217, :374-394).
 */
#ifndef MONORUN_TRAIN_H_
#define MONORUN_TRAIN_H_

#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The NOC head's training decode (monorun_roi_head.py:189-217, :374-394 of the reference): from the head's raw output to coords_3d and the
 * pixel log-std, one launch forward and one backward.  Per object i of n and pixel p of h * w, with c = class_agnostic ? 0 : labels[i],
 * f = flip[i] ? 1 : 0, Cn = class_agnostic ? 1 : num_classes, sigma / mu = dim_stds / dim_means[labels[i]], s / m = noc_stds / noc_means,
 * sd = (float)proj_scaling_denominator, k_epi = (float)((ref_focal_y * epistemic_std_gain)^2), k_sd2 = (float)(proj_scaling_denominator^2):
 *   noc_pred_k     = all_pred[i, f 5 Cn + 3 c + k]               k < 3      (fcn_noc_decoder.py:225-267)
 *   proj_logstd_j  = all_pred[i, f 5 Cn + 3 Cn + 2 c + j]        j < 2
 *   dims_k         = dim_k sigma_k + mu_k,   dims_var_k = dim_var_k (sigma_k sigma_k)          (multiclass_norm_dim_coder.py:28-36)
 *   part_k         = noc_pred_k s_k + m_k,   coords_3d_k = part_k dims_k,   coords_3d_var_k = dims_var_k (part_k part_k)   (noc_coder.py:50-73)
 *   d              = distances ? (distances[i] < distance_min ? distance_min : distances[i]) : sd
 *   with dim_var:    proj_logstd_px_j = 0.5 mr_logf((var2d_j k_epi + mr_expf(2 proj_logstd_j) k_sd2) / (d d)),
 *                    var2d = (0.5 (coords_3d_var_0 + coords_3d_var_2), coords_3d_var_1)        (distance_invar_proj_error_coder.py:39-60)
 *   without:         proj_logstd_px_j = proj_logstd_j + mr_logf(sd / d)
 * in fp32, every multiplication, addition and division a separate IEEE operation in this order; mr_expf / mr_logf are the library's
 * specified exp / log.  coords_3d, dims and dims_var are bit-identical to mr_noc_decode_batched's, and with distances = NULL
 * mr_expf(-proj_logstd_px) / std_scale is its coords_2d_istd.
 *
 * Inputs (device): all_pred (n, 2 Cn 5, h, w) contiguous, pred_dtype MR_F32, MR_F16 or MR_BF16; labels (n) int64 in [0, num_classes)
 * (not checked: the host cannot); flip (n) uint8_t; dim (n, 3) fp32; dim_var (n, 3) fp32 or NULL (no variance: coords_3d_var, dims_var
 * and grad_dim_var are not written and may be NULL); distances (n) fp32 or NULL; dim_means, dim_stds (num_classes, 3), noc_means,
 * noc_stds (3) fp32.
 * Outputs (device, fp32, contiguous, all required but the two the variance needs): noc_pred, coords_3d, coords_3d_var (n, 3, h, w);
 * proj_logstd, proj_logstd_px (n, 2, h, w); dims, dims_var (n, 3).
 *
 * n = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for n < 0, h < 1, w < 1, num_classes < 1 or a NULL required pointer,
 * MR_ERR_UNSUPPORTED for another pred_dtype or more than 2^31 - 1 workgroups.
 */
int mr_noc_decode_train(const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                        const float *dim_var, const float *distances, int n, int num_classes, int class_agnostic, int h, int w,
                        const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                        double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, double distance_min,
                        float *noc_pred, float *proj_logstd, float *coords_3d, float *coords_3d_var, float *proj_logstd_px,
                        float *dims, float *dims_var, void *stream);

/*
 * mr_noc_decode_train_backward: the gradients of mr_noc_decode_train's outputs to all_pred, dim and dim_var, ONE launch (a workgroup
 * per object) that recomputes the forward from the same inputs; nothing else is saved.  The distances do not enter: d only adds a
 * constant to proj_logstd_px.  grad_noc_pred, grad_proj_logstd, grad_coords_3d, grad_coords_3d_var, grad_proj_logstd_px (the maps' shapes)
 * and grad_dims, grad_dims_var (n, 3) are the upstream gradients, fp32 contiguous; each may be NULL, meaning zero (grad_coords_3d_var
 * and grad_dims_var are ignored without dim_var).  Per pixel, with t_j = var2d_j k_epi + mr_expf(2 proj_logstd_j) k_sd2:
 *   g_ls_j   = grad_proj_logstd_j + grad_proj_logstd_px_j (mr_expf(2 proj_logstd_j) k_sd2) / t_j        (without dim_var: the plain sum)
 *   g_v2d_j  = grad_proj_logstd_px_j (0.5 k_epi) / t_j
 *   g_var_k  = grad_coords_3d_var_k + (k == 1 ? g_v2d_1 : 0.5 g_v2d_0)
 *   g_part_k = grad_coords_3d_k dims_k + 2 g_var_k dims_var_k part_k,      g_noc_k = grad_noc_pred_k + g_part_k s_k
 * Outputs: grad_all_pred (n, 2 Cn 5, h, w) in all_pred's dtype — EVERY element is written, the five selected channels of an object with
 * g_noc / g_ls and all others with 0, so the buffer needs no memset; grad_dim (n, 3) fp32 = (grad_dims_k + sum_p grad_coords_3d_k part_k)
 * sigma_k and, with dim_var, grad_dim_var (n, 3) fp32 = (grad_dims_var_k + sum_p g_var_k part_k^2) (sigma_k sigma_k): the sums in fp64,
 * per thread, then over the wave and the four waves in a fixed order.  No atomics, no workspace: bitwise reproducible.
 *
 * n = 0 launches nothing and returns 0.  Errors as mr_noc_decode_train; grad_all_pred and grad_dim are required, grad_dim_var with dim_var.
 */
int mr_noc_decode_train_backward(const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                                 const float *dim_var, int n, int num_classes, int class_agnostic, int h, int w,
                                 const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                                 double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain,
                                 const float *grad_noc_pred, const float *grad_proj_logstd, const float *grad_coords_3d,
                                 const float *grad_coords_3d_var, const float *grad_proj_logstd_px, const float *grad_dims,
                                 const float *grad_dims_var, void *grad_all_pred, float *grad_dim, float *grad_dim_var, void *stream);

#ifdef __cplusplus
}
#endif
#endif
