/*
 * monorun_assign.h — C ABI of the 2-D detector's target assignment in libmonorun_pnp.so: mmdet 2.x's MaxIoUAssigner (with
 * gt_max_assign_all = True and ignore_wrt_candidates = True) and DeltaXYWHBBoxCoder.encode for all images of a batch, TWO launches
 * (DESIGN.md section 21).  The entry points are compiled into the same library as those of monorun_pnp.h and follow its conventions: 0 on
 * success or a negative MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernels, in
 * stream order, unless it is called a HOST array below (read before the call returns); a call runs on the current HIP device,
 * asynchronously on `stream`; nothing is allocated and nothing synchronises, so a call can be captured into a graph.
 *
 * Reference interface replaced: mmdet.core.bbox.assigners.MaxIoUAssigner.assign with BboxOverlaps2D, and bbox2delta, as
 * AnchorHead.get_targets and MonoRUnRoIHead.forward_train call them once per image.
 */
#ifndef MONORUN_ASSIGN_H_
#define MONORUN_ASSIGN_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ASSIGN_MAX_GT 256            /* ground truths of one image: 4 KB of LDS, read as broadcasts */
#define MR_ASSIGN_MAX_IGNORE 256        /* ignore boxes of one image: 4 KB of LDS */
#define MR_ASSIGN_MAX_IMAGES 65535      /* gridDim.y */
#define MR_ASSIGN_THREADS 256           /* boxes of one block, one per thread */
#define MR_ASSIGN_MAX_LDS_BYTES (MR_ASSIGN_MAX_GT * 16 + MR_ASSIGN_MAX_IGNORE * 16 + MR_ASSIGN_MAX_GT * 4)      /* gt, ignore, the block's gt_max keys */
#define MR_ASSIGN_FINISH_LDS_BYTES (MR_ASSIGN_MAX_GT * 16 + MR_ASSIGN_MAX_GT * 4)                                /* gt, gt_max */

/*
 * The overlap, every operation rounded to fp32, no contraction, an IEEE division, eps = 1e-6f; min and max return a NaN operand
 * (torch's, not fminf's):
 *   area = (x2 - x1)(y2 - y1);  w = max(min(ax2, bx2) - max(ax1, bx1), 0), h alike;  inter = w h
 *   iou = inter / max((area_a + area_b) - inter, eps);   iof = inter / max(area_a, eps), a the candidate box
 * This is not the NMS rule of monorun_proposals.h, which has no eps.
 *
 * The bytes of mr_assign_max_iou's workspace: 4 n_images max_gt (the gt_max keys); 0 for a negative argument.
 */
size_t mr_assign_workspace_bytes(int n_images, int max_gt);

/*
 * mr_assign_max_iou: the assignment of every box of every image and its regression target.
 *
 * boxes: box b of image n is the four floats at boxes + n image_stride + b box_stride (strides in floats; box_stride 4 or 5, image_stride
 * 0 for one set of boxes shared by all images or >= n_boxes box_stride); valid (n_images, n_boxes) uint8 or NULL; counts (n_images,) int32
 * or NULL.  Box b of image n is ABSENT if valid says 0 or b >= counts[n]: it is never read, takes part in nothing and gets gt_ind -1,
 * max_overlap 0, argmax 0, ignored 0, label -1, deltas 0.  gt_bboxes (sum G, 4) fp32 and gt_labels (sum G,) int32 or NULL, image n's at
 * rows gt_offsets[n] .. gt_offsets[n + 1] - 1 (gt_offsets (n_images + 1,) int32); ignore_bboxes / ignore_offsets alike, both NULL for
 * none.  max_gt, max_ignore: HOST bounds of the per-image counts; an image with more is cut to its first max_gt (max_ignore) in both
 * kernels alike.  means, stds: HOST arrays of 4.
 *
 * Per image with G > 0 ground truths, over its present boxes:
 *   1. with ignore_iof_thr > 0 and ignore boxes, a box whose largest iof over them is > ignore_iof_thr is IGNORED: all its overlaps are -1
 *   2. max_overlap[b], argmax[b]: the largest iou over the ground truths from a running maximum that starts at (-1, 0) and is raised by
 *      `>` only: ties go to the lower ground truth, a NaN never raises it
 *   3. gt_max[i]: the largest overlap of ground truth i over the present boxes, from -1 by `>` likewise (a zero is +0)
 *   4. gt_ind = -1;  0 where 0 <= max_overlap < neg_iou_thr;  argmax + 1 where max_overlap >= pos_iou_thr
 *   5. with match_low_quality, for i ascending: where overlap(i, b) == gt_max[i] and gt_max[i] >= min_pos_iou, gt_ind = i + 1 (the last
 *      i wins)
 *   6. label = gt_labels[gt_ind - 1] (0 with gt_labels NULL) where gt_ind > 0, else -1
 *   deltas = ((d - mean) / std) of d = [(gx - px) / pw, (gy - py) / ph, logf(gw / pw), logf(gh / ph)], px = (x1 + x2) 0.5, pw = x2 - x1
 *   (y alike) for the box p and its ground truth g, where gt_ind > 0, else 0
 * An image with G = 0: gt_ind 0, max_overlap 0, argmax 0, ignored 0, label -1, deltas 0 for every present box.
 *
 * Outputs: max_overlap (n_images, n_boxes) fp32, argmax int32, ignored uint8, gt_ind int32, label int32 (or NULL), deltas (n_images,
 * n_boxes, 4) fp32 (or NULL); gt_max (sum G,) fp32 in gt_bboxes' layout (or NULL; the entries of a cut image past max_gt are not
 * written).  workspace: mr_assign_workspace_bytes bytes, 4-byte aligned; it is cleared by a memset on `stream` inside the call.
 *
 * The first launch combines the blocks' shares of gt_max with one integer atomicMax per block and ground truth on the overlap's bit
 * pattern plus one (non-negative floats order as their bit patterns; 0 stays "none"): a maximum is exact in any order, so the result is
 * bitwise a function of the inputs.  The second launch recomputes each box's row with the same device routine, so `==` compares
 * identical values.
 *
 * n_images = 0 or n_boxes = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for a negative count, a box_stride other than 4 or 5,
 * a negative image_stride or one in (0, n_boxes box_stride), a NULL required pointer (with max_gt = 0 gt_bboxes may be NULL; gt_offsets
 * may not; label, deltas, gt_max, gt_labels, valid and counts are optional), or ignore_bboxes without ignore_offsets with max_ignore > 0;
 * MR_ERR_UNSUPPORTED for max_gt > MR_ASSIGN_MAX_GT, max_ignore > MR_ASSIGN_MAX_IGNORE, n_images > MR_ASSIGN_MAX_IMAGES or n_images n_boxes
 * > 2^31 - 1.
 */
int mr_assign_max_iou(const float *boxes, int64_t image_stride, int box_stride, const uint8_t *valid, const int32_t *counts, int n_images,
                      int n_boxes, const float *gt_bboxes, const int32_t *gt_offsets, const int32_t *gt_labels, int max_gt,
                      const float *ignore_bboxes, const int32_t *ignore_offsets, int max_ignore, float pos_iou_thr, float neg_iou_thr,
                      float min_pos_iou, float ignore_iof_thr, int match_low_quality, const float *means, const float *stds,
                      float *max_overlap, int32_t *argmax, uint8_t *ignored, float *gt_max, int32_t *gt_ind, int32_t *label, float *deltas,
                      void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
