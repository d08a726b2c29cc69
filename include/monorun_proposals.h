/*
 * monorun_proposals.h — C ABI of the proposal stage in libmonorun_pnp.so: the RPN's fused proposal decode and the grouped axis-aligned
 * NMS that mmdet's RPNHead.get_bboxes and multiclass_nms end in (mmcv.ops.nms / batched_nms).  The entry points
 * are compiled into the same library as those of monorun_pnp.h and follow its conventions: 0 on success or a negative MR_ERR_* code of
 * monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernels, in stream order, unless it is called a HOST
 * array below (read before the call returns); a call runs on the current HIP device, asynchronously on `stream`; nothing is allocated.
 *
 * Reference interface replaced: mmdet.models.dense_heads.RPNHead.get_bboxes (the reference's RPNHeadMod inherits it) with
 * DeltaXYWHBBoxCoder.decode, and mmcv.ops.nms / batched_nms, a CUDA extension with no ROCm build.
 */
#ifndef MONORUN_PROPOSALS_H_
#define MONORUN_PROPOSALS_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_PROPOSAL_MAX_LEVELS 8        /* n_levels */
#define MR_PROPOSAL_MAX_ANCHORS 16      /* n_anchors: base anchors per level */
#define MR_NMS_MAX_GROUP 4096           /* boxes of one group: 64 lanes x 64 bits, the scan's removed set */
#define MR_NMS_MAX_GROUPS 65535         /* groups of one call */
#define MR_NMS_TILE 64                  /* the suppression matrix is computed in 64 x 64 tiles of 64-bit words */
#define MR_NMS_SCAN_ROWS 32             /* rows of the matrix the scan holds per register buffer (it has two) */
#define MR_PROPOSAL_DECODE_LDS_BYTES 0
#define MR_NMS_MASK_LDS_BYTES (MR_NMS_TILE * 16)    /* the tile's 64 column boxes */
#define MR_NMS_SCAN_LDS_BYTES 0

/*
 * mr_proposal_decode: mmdet's delta2bbox on the selected candidates of every (image, level), ONE launch.  cls[l] (n_images, n_anchors,
 * level_h[l], level_w[l]) and reg[l] (n_images, 4 n_anchors, level_h[l], level_w[l]) fp32 contiguous, the head's NCHW outputs as they
 * are; cls, reg, level_h, level_w, level_stride, level_count (n_levels entries each), base_anchors (n_levels, n_anchors, 4), means (4)
 * and stds (4) are HOST arrays: the level table travels in the kernel arguments.  index (n_images, sum_l level_count[l]) int64: per image
 * the level_count[l] selected flat anchor indices t = (y W_l + x) n_anchors + a of level 0 in rank order, then level 1's, ...;
 * img_shape (n_images, 2) fp32 = [img_h, img_w].  Outputs in index's layout, T = n_images sum_l level_count[l]: boxes (T, 4), score (T,),
 * logit (T,) fp32, valid (T,) uint8.  Per candidate, every operation rounded to fp32, no contraction:
 *   anchor = base_anchors[l][a] + (x s, y s, x s, y s), s = level_stride[l];   logit = cls[l][n, a, y, x];  delta_c = reg[l][n, 4 a + c, y, x]
 *   d = delta std + mean;  dw, dh clamped to +-max_ratio, max_ratio = (float)|log(wh_ratio_clip)|
 *   px = (x1 + x2) 0.5, pw = x2 - x1;  gw = pw expf(dw), gx = px + pw dx;  x1' = gx - gw 0.5, x2' = gx + gw 0.5   (y alike)
 *   x' clamped to [0, img_w], y' to [0, img_h];  valid = !(min_bbox_size > 0 && (x2' - x1' < min_bbox_size || y2' - y1' < min_bbox_size))
 *   score = 1 / (1 + expf(-logit))
 * An index outside [0, H_l W_l n_anchors) reads nothing and gives NaN boxes, score and logit and valid 0.
 *
 * No candidates (every level_count 0) launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for n_levels, n_images, n_anchors, a level
 * size or stride < 1, a level_count < 0, a wh_ratio_clip that is not positive and finite, or a NULL pointer; MR_ERR_UNSUPPORTED for
 * n_levels > MR_PROPOSAL_MAX_LEVELS, n_anchors > MR_PROPOSAL_MAX_ANCHORS, a head output or T of more than 2^31 - 1 elements, or n_images
 * n_levels > 65535.
 */
int mr_proposal_decode(const float *const *cls, const float *const *reg, const int *level_h, const int *level_w, const int *level_stride,
                       const int *level_count, const float *base_anchors, int n_levels, int n_anchors, int n_images, const int64_t *index,
                       const float *img_shape, const float *means, const float *stds, double wh_ratio_clip, float min_bbox_size,
                       float *boxes, float *score, float *logit, uint8_t *valid, void *stream);

/*
 * The bytes of mr_nms_grouped's workspace: 8 sum_g n_g ceil(n_g / 64) for the group sizes n_g = group_sizes[g] (a HOST array; sizes
 * above max_group count as max_group, as the kernels read them).  0 for no groups or a NULL or negative argument.
 */
size_t mr_nms_workspace_bytes(const int *group_sizes, int groups, int max_group);

/*
 * mr_nms_grouped: greedy axis-aligned NMS inside each group, TWO launches (the suppression bit matrix, then one wave per group that
 * scans it), no atomics, no host synchronisation; the result is bitwise a function of the inputs.  boxes (T, 4) fp32 [x1, y1, x2, y2],
 * in rank order inside each group; valid (T,) uint8 or NULL (all valid); offsets (groups + 1,) int32, group g = boxes offsets[g] ..
 * offsets[g + 1] - 1; max_group: a HOST bound of the group sizes, which sizes the grid (a group larger than it is cut to its first
 * max_group boxes, the others get keep 0).  Box i is kept iff it is valid and no kept box j < i of its group has iou(j, i) > thr, with
 *   iw = max(min(ax2, bx2) - max(ax1, bx1), 0), ih alike;  inter = iw ih;  area = (x2 - x1)(y2 - y1);  iou = inter / ((area_a + area_b) - inter)
 * every operation rounded to fp32, no contraction, an IEEE division (mmcv's offset = 0).  A NaN iou does not suppress.  keep (T,) uint8
 * (only the entries of the groups are written); num_keep (groups,) int32; workspace: mr_nms_workspace_bytes bytes, 8-byte aligned.
 *
 * groups = 0 or max_group = 0 (no boxes) launches nothing, writes nothing and returns 0.
 * MR_ERR_BAD_ARGUMENT for a negative count or a NULL pointer (valid excepted); MR_ERR_UNSUPPORTED for max_group > MR_NMS_MAX_GROUP or
 * groups > MR_NMS_MAX_GROUPS.
 */
int mr_nms_grouped(const float *boxes, const uint8_t *valid, const int32_t *offsets, int groups, int max_group, float thr,
                   uint8_t *keep, int32_t *num_keep, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
