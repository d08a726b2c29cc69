/*
 * monorun_bbox.h — C ABI of the 2-D detection head's get_bboxes in libmonorun_pnp.so: softmax, delta2bbox per class, NMS per (image,
 * class) and the per-image top max_num, as mmdet's Shared2FCBBoxHead.get_bboxes and multiclass_nms compute them.
 * The entry points are compiled into the same library as those of monorun_pnp.h and follow its conventions: 0 on success or a negative
 * MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernels, in stream order, unless it is
 * called a HOST array below (read before the call returns); a call runs on the current HIP device, asynchronously on `stream`; nothing is
 * allocated; every check comes before any HIP call.
 *
 * Reference interface replaced: mmdet.models.roi_heads.bbox_heads.BBoxHead.get_bboxes (F.softmax, DeltaXYWHBBoxCoder.decode, the rescale)
 * and mmdet.core.post_processing.multiclass_nms, which ends in mmcv.ops.batched_nms, a CUDA extension with no ROCm build.
 *
 * The stage is FOUR launches: mr_bbox_head_rank, the two of mr_nms_grouped (monorun_proposals.h), mr_bbox_head_select; no atomics, no
 * host synchronisation; every output is bitwise a function of the inputs.
 *
 * Common arguments.  n_rois = R rows in all, image-major; n_images = N; num_classes = C; row_offsets (N + 1,) int32: image n owns the rows
 * row_offsets[n] .. row_offsets[n + 1] - 1.  Every kernel reads them alike: cut to [0, R], made monotone, and the count K_n cut to
 * max_rois, a HOST bound of the rows of one image — so that a wrong bound cannot send a kernel out of a buffer (the rows past it take no
 * part).  The candidates are laid out in groups (n, c), image-major, T = R C places in all: group (n, c) starts at C row_offsets[n] + c K_n
 * and holds the K_n rows of image n in rank order for class c.
 */
#ifndef MONORUN_BBOX_H_
#define MONORUN_BBOX_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"
#include "monorun_proposals.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_BBOX_MAX_ROIS 4096           /* max_rois: the rows of one image = MR_NMS_MAX_GROUP; the rank launch sorts them in LDS */
#define MR_BBOX_MAX_CLASSES 16          /* num_classes (without the background) */
#define MR_BBOX_MAX_IMAGES 4095         /* n_images: n_images num_classes groups <= MR_NMS_MAX_GROUPS */
#define MR_BBOX_RANK_LDS_BYTES (MR_BBOX_MAX_ROIS * 8)                           /* one 64-bit key per row */
#define MR_BBOX_SELECT_LDS_BYTES (MR_BBOX_MAX_CLASSES * (MR_BBOX_MAX_ROIS / 64) * 12)  /* per class 64 words of kept flags, a count each */

/*
 * mr_bbox_head_rank: ONE launch, a workgroup per (image, class).  cls_score (R, C + 1) fp32 logits, the background last; bbox_pred
 * (R, 4 C), or (R, 4) with reg_class_agnostic; rois (R, 5) [image, x1, y1, x2, y2] (column 0 is not read: row_offsets says whose a row
 * is); img_shape (N, 2) fp32 [img_h, img_w]; scale_factor (N, 4) fp32 or NULL (no rescale); means (4), stds (4): HOST arrays.  Per row r of
 * image n and class c, every operation rounded to fp32, no contraction:
 *   m = max_j x_j;  e_j = expf(x_j - m);  s = e_0 + e_1 + ... + e_C in index order;  score = e_c / s
 *   d = delta std + mean (delta = bbox_pred[r, 4c .. 4c + 3], columns 0 .. 3 when class-agnostic);  dw, dh clamped to +-max_ratio,
 *   max_ratio = (float)|log(wh_ratio_clip)|;  px = (x1 + x2) 0.5, pw = x2 - x1;  gw = pw expf(dw), gx = px + pw dx;
 *   x1' = gx - gw 0.5, x2' = gx + gw 0.5 (y alike);  x' clamped to [0, img_w], y' to [0, img_h];  with scale_factor, x1' / f0, y1' / f1,
 *   x2' / f2, y2' / f3
 *   valid = score > score_thr and x1, y1, x2, y2 of the RoI all finite (a NaN score compares false)
 * Ranks inside group (n, c): score descending, NaN scores after every number, ties to the lower row, over all K_n rows whatever their
 * validity.  Outputs in the groups' layout: boxes (T, 4), score (T,) fp32 (a NaN score is written as the canonical quiet NaN), order (T,)
 * int32 (the row inside its image), valid (T,) uint8; group_offsets (N C + 1,) int32, the offsets mr_nms_grouped takes.  Places no group
 * covers are not written.  The box of a row whose RoI is not finite is unspecified (it is not valid).
 */
int mr_bbox_head_rank(const float *cls_score, const float *bbox_pred, const float *rois, const int32_t *row_offsets, const float *img_shape,
                      const float *scale_factor, int n_rois, int n_images, int num_classes, int reg_class_agnostic, int max_rois,
                      const float *means, const float *stds, double wh_ratio_clip, float score_thr, float *boxes, float *score,
                      int32_t *order, uint8_t *valid, int32_t *group_offsets, void *stream);

/*
 * mr_bbox_head_select: ONE launch, a workgroup per image.  boxes, score, order: the rank launch's outputs; keep (T,) uint8: the NMS's
 * flags in the same layout.  Per image the kept candidates by score descending, ties to the lower candidate index order C + c, the first
 * max_num: dets (N, max_num, 5) fp32 [x1, y1, x2, y2, score], labels (N, max_num) int64 = c, counts (N,) int32; rows past the count are
 * NaN and their labels -1.  The scores of the kept candidates must be numbers (those of valid candidates are).
 */
int mr_bbox_head_select(const float *boxes, const float *score, const int32_t *order, const uint8_t *keep, const int32_t *row_offsets,
                        int n_rois, int n_images, int num_classes, int max_rois, int max_num, float *dets, int64_t *labels, int32_t *counts,
                        void *stream);

/* The bytes of mr_bbox_head_detect's workspace (8-byte aligned); 0 for a negative argument or num_classes < 1. */
size_t mr_bbox_head_workspace_bytes(int n_rois, int n_images, int num_classes, int max_rois);

/*
 * mr_bbox_head_detect: the four launches: mr_bbox_head_rank, mr_nms_grouped with threshold iou_thr on the groups (n, c) with the rank
 * launch's valid flags, mr_bbox_head_select.  The intermediate arrays live in `workspace`.
 *
 * All three: n_rois = 0, n_images = 0 or max_rois = 0 launches nothing, writes nothing and returns 0 (the caller fills dets, labels and
 * counts).  MR_ERR_BAD_ARGUMENT for a negative count, num_classes < 1, max_num < 1, a wh_ratio_clip that is not positive and finite or a
 * NULL pointer (scale_factor excepted); MR_ERR_UNSUPPORTED for max_rois > MR_BBOX_MAX_ROIS, num_classes > MR_BBOX_MAX_CLASSES, n_images >
 * MR_BBOX_MAX_IMAGES, or 4 n_rois num_classes or 5 n_images max_num above 2^31 - 1.
 */
int mr_bbox_head_detect(const float *cls_score, const float *bbox_pred, const float *rois, const int32_t *row_offsets, const float *img_shape,
                        const float *scale_factor, int n_rois, int n_images, int num_classes, int reg_class_agnostic, int max_rois,
                        const float *means, const float *stds, double wh_ratio_clip, float score_thr, float iou_thr, int max_num,
                        float *dets, int64_t *labels, int32_t *counts, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
