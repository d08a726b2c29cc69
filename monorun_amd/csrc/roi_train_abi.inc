// include/monorun_roi_train.h: the positives of a training step, from the 2-D stage's sampling to what the 3-D heads take
int mr_roi_train_positives(const float *bboxes, const int64_t *gt_inds, const int64_t *labels, const int64_t *pos_inds,
                           const int32_t *pos_offsets, int n_images, int n_boxes, int num, int n_pos, const float *bbox_pred,
                           const int32_t *bbox_row_offsets, int n_rows, int num_classes, int reg_class_agnostic, const float *gt_bboxes_3d,
                           const int32_t *gt_offsets, int n_gt, int max_gt, const float *cam_intrinsic, const float *img_shape,
                           const uint8_t *flip, const float *means, const float *stds, double wh_ratio_clip, const float *dim_means,
                           const float *dim_stds, float *pos_rois, float *pos_bboxes, int64_t *pos_gt_labels, int64_t *pos_assigned_gt_inds,
                           int32_t *pos_img, int64_t *pos_img_long, float *pos_bboxes_3d, float *pos_cam_intrinsic, float *pos_img_shapes,
                           uint8_t *pos_flip, float *dim_targets, void *stream) {
    static_assert(kRoiTrainThreads == MR_ROI_TRAIN_THREADS && kAssignMaxImages == MR_ROI_TRAIN_MAX_IMAGES && kAssignMaxGt == MR_ROI_TRAIN_MAX_GT &&
                  kBboxMaxClasses == MR_ROI_TRAIN_MAX_CLASSES, "the header states the caps");
    if (n_images < 0 || n_boxes < 0 || num < 0 || n_pos < 0 || n_rows < 0 || num_classes < 1 || n_gt < 0 || max_gt < 0) return MR_ERR_BAD_ARGUMENT;
    if (!means || !stds || !(wh_ratio_clip > 0.0) || !(fabs(log(wh_ratio_clip)) < 1e30)) return MR_ERR_BAD_ARGUMENT;
    if (n_images > kAssignMaxImages || max_gt > kAssignMaxGt || num_classes > kBboxMaxClasses) return MR_ERR_UNSUPPORTED;
    if ((long long)n_images * n_boxes > 0x7fffffffLL || (long long)n_images * num > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    if ((long long)n_rows * num_classes * 4 > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    if (n_pos == 0) return MR_OK;
    if (n_images == 0 || n_pos > (long long)n_images * num) return MR_ERR_BAD_ARGUMENT;      // positives without an image to hold them
    if (!bboxes || !gt_inds || !labels || !pos_inds || !pos_offsets || !bbox_pred || !bbox_row_offsets || !gt_bboxes_3d || !gt_offsets ||
        !cam_intrinsic || !img_shape || !flip || !dim_means || !dim_stds)
        return MR_ERR_BAD_ARGUMENT;
    if (!pos_rois || !pos_bboxes || !pos_gt_labels || !pos_assigned_gt_inds || !pos_img || !pos_img_long || !pos_bboxes_3d ||
        !pos_cam_intrinsic || !pos_img_shapes || !pos_flip || !dim_targets)
        return MR_ERR_BAD_ARGUMENT;
    RoiTrainArgs a;
    memset(&a, 0, sizeof a);
    a.bboxes = bboxes; a.gt_inds = (const long long *)gt_inds; a.labels = (const long long *)labels; a.pos_inds = (const long long *)pos_inds;
    a.pos_offsets = (const int *)pos_offsets; a.N = n_images; a.T = n_boxes; a.num = num; a.K = n_pos;
    a.reg = bbox_pred; a.reg_offsets = (const int *)bbox_row_offsets; a.R = n_rows; a.C = num_classes; a.agnostic = reg_class_agnostic ? 1 : 0;
    a.gt3d = gt_bboxes_3d; a.gt_offsets = (const int *)gt_offsets; a.n_gt = n_gt; a.max_gt = max_gt;
    a.cam = cam_intrinsic; a.img_shape = img_shape; a.flip = flip;
    for (int k = 0; k < 4; ++k) { a.mean[k] = means[k]; a.std[k] = stds[k]; }
    a.max_ratio = (float)fabs(log(wh_ratio_clip));
    a.dim_mean = dim_means; a.dim_std = dim_stds;
    a.rois = pos_rois; a.boxes = pos_bboxes; a.out_labels = (long long *)pos_gt_labels; a.out_gt = (long long *)pos_assigned_gt_inds;
    a.img32 = (int *)pos_img; a.img64 = (long long *)pos_img_long; a.out3d = pos_bboxes_3d; a.out_cam = pos_cam_intrinsic;
    a.out_shape = pos_img_shapes; a.out_flip = pos_flip; a.dim_targets = dim_targets;
    const dim3 grid((unsigned)((n_pos + kRoiTrainThreads - 1) / kRoiTrainThreads));
    hipLaunchKernelGGL(roi_train_positives_kernel, grid, dim3(kRoiTrainThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
