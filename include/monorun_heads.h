/*
 * monorun_heads.h — C ABI of the head kernels of libmonorun_pnp.so that sit behind the PnP on the inference tail.  The entry points
 * are compiled into the same library as those of monorun_pnp.h and follow its conventions: 0 on success or a negative MR_ERR_* code
 * of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernel, in stream order; a call runs on the
 * current HIP device, asynchronously on `stream`; nothing is allocated.
 *
 * Reference interface replaced: MLPScoreHead.forward of the MonoRUn tree
 * (monorun/models/roi_heads/bbox_3d_heads/score_heads/mlp_score_head.py:94-115) in eval mode, with the sigmoid, the mask of failed
 * solves and the 2-D score multiply of monorun/models/roi_heads/monorun_roi_head.py:544-550, for the configuration every shipped
 * config file uses: one pose layer, one fused layer, fusion by addition.
 */
#ifndef MONORUN_HEADS_H_
#define MONORUN_HEADS_H_

#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of mr_score_head_forward */
#define MR_SCORE_SIGMOID 0x1          /* scores = 1 / (1 + mr_expf(-z)) instead of the logit z */

/* limits of mr_score_head_forward */
#define MR_SCORE_MAX_C1 2048
#define MR_SCORE_MAX_C2 1024

/*
 * mr_score_head_forward: ONE launch, per row i of n:
 *   x    = [yaw, t_vec (3), pose_cov[r, c] in torch.tril_indices(4, 4) order (10), dimensions (3)]                    (17)
 *   xn_k = (x_k - mean_k) * scale_k + shift_k
 *   h1   = relu(W1 xn + b1) + reg_fc_out[i]                                                                            (c1)
 *   h2   = relu(W2 h1 + b2)                                                                                            (c2)
 *   z    = w3 . h2 + b3
 *   s    = (flags & MR_SCORE_SIGMOID) ? 1.0f / (1.0f + mr_expf(-z)) : z          (mr_expf: the library's specified exp; IEEE division)
 *   s    = (ret_val && !ret_val[i]) ? +0.0f : s                                  (a select: a failed solve's covariance may be NaN or inf)
 *   s    = (scores_2d && !(ret_val && !ret_val[i])) ? s * scores_2d[i] : s
 *   scores[i] = s
 * fp32 accumulation; relu keeps NaN, as torch's does.  No floating-point atomics and no workspace: a row's result is bitwise
 * reproducible, and its summation order depends on c1 and c2 only, never on n or on the row's position.
 *
 * Inputs, device fp32 unless stated; a row stride is in elements, and row i starts at base + i * stride:
 *   reg_fc_out (n, c1), stride >= c1;  yaw (n, 1), stride >= 1;  t_vec (n, 3), stride >= 3;  dimensions (n, 3), stride >= 3
 *     (unit column stride; the strides exist because the caller indexes views of wider tensors);
 *   pose_cov (n, 4, 4) contiguous;
 *   ret_val (n) uint8_t (torch.bool memory), or NULL: no row is masked;
 *   scores_2d (n) contiguous, or NULL: no multiply;
 *   params: the module's parameters, packed once by the caller into one buffer of `params_numel` floats.  With
 *     c2p = (c2 + 3) / 4 * 4 and r4(v) = (v + 3) / 4 * 4, the sections follow each other in this order:
 *       mean[17] scale[17] shift[17] and 13 zeros                   (64)      scale = weight / sqrt(running_var + eps), shift = bias;
 *                                                                             without the norm: 0, 1, 0
 *       W1t[k * c1 + j] = W1[j][k], k < 17, j < c1, zero padded      (r4(17 * c1))
 *       b1[c1], zero padded                                          (r4(c1))
 *       W2t[k * c2p + j] = W2[j][k], k < c1, j < c2, 0 for j >= c2   (c1 * c2p)
 *       b2[c2p], w3[c2p], both 0 for j >= c2                         (2 * c2p)
 *       b3 and 3 zeros                                               (4)
 *     so params_numel = 64 + r4(17 * c1) + r4(c1) + c1 * c2p + 2 * c2p + 4, and `params` must be 16-byte aligned.
 * Output: scores (n) contiguous.
 *
 * n = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT, before any HIP call, for n < 0, c1 outside [1, MR_SCORE_MAX_C1],
 * c2 outside [1, MR_SCORE_MAX_C2], a row stride shorter than its row, flag bits other than MR_SCORE_SIGMOID, a params_numel that is
 * not the one above, a misaligned `params`, or a NULL required pointer (all but ret_val, scores_2d and stream).
 */
int mr_score_head_forward(const float *reg_fc_out, int64_t reg_fc_out_row_stride, const float *yaw, int64_t yaw_row_stride,
                          const float *t_vec, int64_t t_vec_row_stride, const float *pose_cov, const float *dimensions,
                          int64_t dimensions_row_stride, const uint8_t *ret_val, const float *scores_2d, const float *params,
                          int64_t params_numel, int n, int c1, int c2, int flags, float *scores, void *stream);

#ifdef __cplusplus
}
#endif
#endif
