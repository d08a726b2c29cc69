/*
 * monorun_roi_train.h — C ABI of the training step's hand-over from the 2-D stage to the 3-D heads in libmonorun_pnp.so: for every sampled
 * positive of a batch, its RoI moved by the deltas of its ground-truth class (mmdet's BBoxHead.regress_by_class) and what the global, NOC,
 * projection and pose heads take per positive, ONE launch.  The entry point is compiled into the same library as
 * those of monorun_pnp.h and follows its conventions: 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data pointer is a
 * DEVICE pointer, dereferenced only by the kernel, in stream order, unless it is called a HOST array below (read before the call
 * returns); a call runs on the current HIP device, asynchronously on `stream`; nothing is allocated and nothing synchronises, so a call
 * can be captured into a graph.
 *
 * Reference interface replaced: the per-image loop of MonoRUnRoIHead.forward_train that masks the RoIs, regresses the positives by their
 * class and writes them back, and the per-image walks of UncertProjectionHead.get_properties, FCExtractor.get_targets and the flip list.
 */
#ifndef MONORUN_ROI_TRAIN_H_
#define MONORUN_ROI_TRAIN_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"
#include "monorun_assign.h"
#include "monorun_bbox.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ROI_TRAIN_THREADS 64                             /* positives of one block, one per thread */
#define MR_ROI_TRAIN_MAX_IMAGES MR_ASSIGN_MAX_IMAGES        /* the assignment's caps: what it cannot assign is not handed over */
#define MR_ROI_TRAIN_MAX_GT MR_ASSIGN_MAX_GT
#define MR_ROI_TRAIN_MAX_CLASSES MR_BBOX_MAX_CLASSES

/*
 * mr_roi_train_positives: the K = n_pos sampled positives of the batch, image by image, inside an image by ascending sampled index.
 *
 * The sampling, dense over T = n_boxes boxes per image: bboxes (n_images, T, 4) fp32, gt_inds (n_images, T) int64 (i + 1 for ground truth
 * i), labels (n_images, T) int64, pos_inds (n_images, num) int64, the sampled positives of each image ascending, -1 past its count.
 * pos_offsets (n_images + 1,) int32: positive k belongs to the last image n with pos_offsets[n] <= k and is the image's
 * j = k - pos_offsets[n]-th (the offsets are read cut to [0, n_pos]).  bbox_pred (n_rows, 4 num_classes) fp32, or (n_rows, 4) with
 * reg_class_agnostic: the row of the image's j-th positive is bbox_row_offsets[n] + j (bbox_row_offsets (n_images,) int32; the reference
 * orders an image's rows positives first).  gt_bboxes_3d (n_gt, 7) fp32 [l, h, w, x, y, z, yaw], image n's at rows gt_offsets[n] ..
 * gt_offsets[n + 1] - 1 (gt_offsets (n_images + 1,) int32); max_gt: a HOST bound of the per-image count, an image with more is cut to its
 * first max_gt.  cam_intrinsic (n_images, 3, 3) fp32, img_shape (n_images, 2) fp32 [img_h, img_w], flip (n_images,) uint8.  means, stds:
 * HOST arrays of 4, the box coder's; wh_ratio_clip its clip.  dim_means, dim_stds (num_classes, 3) fp32, the dimension coder's.
 *
 * Per positive k with sampled index t = pos_inds[n, j], label c = labels[n, t] and ground truth g = gt_inds[n, t] - 1, every operation
 * rounded to fp32, no contraction, IEEE division, in the order monorun_proposals.h states delta2bbox (one device routine serves both):
 *   d = bbox_pred[row, 4c : 4c + 4] (columns 0 : 4 when class-agnostic) std + mean;  dw, dh clamped to +-|log(wh_ratio_clip)|
 *   box = the corners of centre (p + pw dx, ..) and size (pw expf(dw), ..) of p = bboxes[n, t], clamped to [0, img_w] x [0, img_h]
 *   pos_bboxes[k] = box,  pos_rois[k] = [n, box];  positives that are prepended ground truths are moved like any other
 *   pos_gt_labels[k] = c,  pos_assigned_gt_inds[k] = g,  pos_img[k] = pos_img_long[k] = n
 *   pos_bboxes_3d[k] = gt_bboxes_3d[gt_offsets[n] + g],  pos_cam_intrinsic[k] = cam_intrinsic[n],  pos_img_shapes[k] = img_shape[n],
 *   pos_flip[k] = flip[n] != 0,  dim_targets[k] = (pos_bboxes_3d[k, 0 : 3] - dim_means[c]) / dim_stds[c]
 * A positive one of whose indices leaves its table — j past num or the image's share of the offsets, t outside [0, n_boxes), c outside
 * [0, num_classes), g outside the image's first max_gt ground truths or its row outside [0, n_gt), the delta row outside [0, n_rows) — is
 * VOID: nothing is read through that index; its boxes, 3-D box and dimension targets are 0, its label and ground truth -1; image, camera
 * matrix, shape and flip flag are still its image's.
 *
 * Outputs: pos_rois (K, 5), pos_bboxes (K, 4) fp32; pos_gt_labels, pos_assigned_gt_inds, pos_img_long (K,) int64; pos_img (K,) int32;
 * pos_bboxes_3d (K, 7), pos_cam_intrinsic (K, 3, 3), pos_img_shapes (K, 2), dim_targets (K, 3) fp32; pos_flip (K,) uint8.  One thread per
 * positive writes every element of its rows once: no atomics, the result is bitwise a function of the inputs.
 *
 * n_pos = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for a negative count, num_classes < 1, NULL means or stds, a
 * wh_ratio_clip that is not a positive finite number, n_pos > n_images num, or a NULL data pointer with n_pos > 0; MR_ERR_UNSUPPORTED for
 * n_images > MR_ROI_TRAIN_MAX_IMAGES, max_gt > MR_ROI_TRAIN_MAX_GT, num_classes > MR_ROI_TRAIN_MAX_CLASSES, or n_images n_boxes,
 * n_images num or 4 n_rows num_classes > 2^31 - 1.
 */
int mr_roi_train_positives(const float *bboxes, const int64_t *gt_inds, const int64_t *labels, const int64_t *pos_inds,
                           const int32_t *pos_offsets, int n_images, int n_boxes, int num, int n_pos, const float *bbox_pred,
                           const int32_t *bbox_row_offsets, int n_rows, int num_classes, int reg_class_agnostic, const float *gt_bboxes_3d,
                           const int32_t *gt_offsets, int n_gt, int max_gt, const float *cam_intrinsic, const float *img_shape,
                           const uint8_t *flip, const float *means, const float *stds, double wh_ratio_clip, const float *dim_means,
                           const float *dim_stds, float *pos_rois, float *pos_bboxes, int64_t *pos_gt_labels, int64_t *pos_assigned_gt_inds,
                           int32_t *pos_img, int64_t *pos_img_long, float *pos_bboxes_3d, float *pos_cam_intrinsic, float *pos_img_shapes,
                           uint8_t *pos_flip, float *dim_targets, void *stream);

#ifdef __cplusplus
}
#endif
#endif
