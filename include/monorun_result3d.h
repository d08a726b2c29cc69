/*
 * monorun_result3d.h — C ABI of the per-image result tail in libmonorun_pnp.so: from the poses and their scores to the class-grouped,
 * NMS-filtered 3-D rows and the matching 2-D boxes, ONE launch.  The entry point is compiled into the same
 * library as those of monorun_pnp.h and follows its conventions: 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data
 * pointer is a DEVICE pointer, dereferenced only by the kernel, in stream order; a call runs on the current HIP device, asynchronously
 * on `stream`; nothing is allocated and nothing synchronises, so a call can be captured into a graph.
 *
 * Reference interface replaced: MonoRUnRoIHead.get_bbox_3d_result, multiclass_3d_result_nms (with xywhr2xyxyr and
 * mmdet3d.ops.iou3d.nms_gpu) and the per-class selection of the 2-D boxes that follows them in simple_test.
 */
#ifndef MONORUN_RESULT3D_H_
#define MONORUN_RESULT3D_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_RESULT3D_MAX_N 512           /* rows of one call: a class may hold all of them, and the NMS keeps a group's removed set in one wave, 16 words of 32 */
#define MR_RESULT3D_MAX_CLASSES 16      /* classes of one call: one workgroup each */
#define MR_RESULT3D_THREADS 256         /* threads of a workgroup */
#define MR_RESULT3D_BOX_BYTES 44        /* one box of the NMS: centre, four corners, area */
/*
 * Dynamic LDS of a launch over n rows, np2 the power of two >= max(n, 1): sort keys and indices (8 np2), boxes (44 n), suppression bits
 * (4 n ceil(n / 32)), 16 bytes of counters, the members' rows (4 n).  The first four terms are mr_nms_bev_batched's for a group of n.
 */
#define MR_RESULT3D_LDS_BYTES(n, np2) ((np2) * 8 + (n) * MR_RESULT3D_BOX_BYTES + (n) * (((n) + 31) / 32) * 4 + 16 + (n) * 4)
#define MR_RESULT3D_MAX_LDS_BYTES MR_RESULT3D_LDS_BYTES(MR_RESULT3D_MAX_N, 512)

/*
 * mr_result3d_nms: per class c < num_classes, the rows of that class after the rotated-BEV NMS, in the order the NMS keeps them.
 *
 * Inputs, fp32 and contiguous unless said: dimensions (n, 3) [l, h, w], yaw (n, 1), t_vec (n, 3) [x, y, z], scores (n,), labels (n,)
 * int64, det_bboxes (n, 5).
 *
 * The MEMBERS of class c are the rows r with labels[r] == c in ascending r; a member's LOCAL INDEX is the number of members before it.
 * A row with a negative label or one >= num_classes belongs to no class.  A member's BEV box is [x - l / 2, z - w / 2, x + l / 2,
 * z + w / 2, yaw], each of the four a single fp32 subtraction or addition of the fp32 half: the boxes of mr_nms_bev_batched given the
 * same numbers.  The NMS is mr_nms_bev_batched's: visiting order by descending score, equal scores by ascending local index, NaN
 * scores last; a box is dropped when its IoU with a kept earlier one is > thr.
 *
 * Outputs; every element is stored exactly once, so the caller need not clear them:
 *   out3d (num_classes, n, 8) fp32, 16-byte aligned: [l, h, w, x, y, z, yaw, score] of the k-th kept member of class c at (c, k)
 *   out2d (num_classes, n, 5) fp32: its det_bboxes row
 *   keep_local (num_classes, n) int64: its local index;  keep_row (num_classes, n) int64: its row
 *   num_keep (num_classes,) int32: the number kept;  num_in_class (num_classes,) int32: the number of members
 * Places k >= num_keep[c] hold NaN in out3d and out2d and -1 in keep_local and keep_row.  The result is bitwise a function of the
 * inputs: no atomics, one fixed order of every sum.
 *
 * num_classes = 0 launches nothing and returns 0; n = 0 stores the two counts.  MR_ERR_BAD_ARGUMENT for a negative count, a NULL
 * output, a NULL input with n > 0, or an out3d that is not 16-byte aligned; MR_ERR_UNSUPPORTED for n > MR_RESULT3D_MAX_N or
 * num_classes > MR_RESULT3D_MAX_CLASSES.
 */
int mr_result3d_nms(const float *dimensions, const float *yaw, const float *t_vec, const float *scores, const int64_t *labels,
                    const float *det_bboxes, int n, int num_classes, float thr, float *out3d, float *out2d, int64_t *keep_local,
                    int64_t *keep_row, int32_t *num_keep, int32_t *num_in_class, void *stream);

#ifdef __cplusplus
}
#endif
#endif
