// include/monorun_assign.h: the 2-D detector's target assignment, mmdet's MaxIoUAssigner and bbox2delta
size_t mr_assign_workspace_bytes(int n_images, int max_gt) {
    if (n_images < 0 || max_gt < 0) return 0;
    return (size_t)n_images * (size_t)max_gt * sizeof(unsigned);
}

int mr_assign_max_iou(const float *boxes, int64_t image_stride, int box_stride, const uint8_t *valid, const int32_t *counts, int n_images,
                      int n_boxes, const float *gt_bboxes, const int32_t *gt_offsets, const int32_t *gt_labels, int max_gt,
                      const float *ignore_bboxes, const int32_t *ignore_offsets, int max_ignore, float pos_iou_thr, float neg_iou_thr,
                      float min_pos_iou, float ignore_iof_thr, int match_low_quality, const float *means, const float *stds,
                      float *max_overlap, int32_t *argmax, uint8_t *ignored, float *gt_max, int32_t *gt_ind, int32_t *label, float *deltas,
                      void *workspace, void *stream) {
    static_assert(kAssignMaxGt == MR_ASSIGN_MAX_GT && kAssignMaxIgnore == MR_ASSIGN_MAX_IGNORE && kAssignThreads == MR_ASSIGN_THREADS &&
                  kAssignMaxImages == MR_ASSIGN_MAX_IMAGES, "the header states the caps");
    static_assert(sizeof(float4) * (kAssignMaxGt + kAssignMaxIgnore) + sizeof(unsigned) * kAssignMaxGt == MR_ASSIGN_MAX_LDS_BYTES &&
                  sizeof(float4) * kAssignMaxGt + sizeof(float) * kAssignMaxGt == MR_ASSIGN_FINISH_LDS_BYTES, "the header states the LDS");
    if (n_images < 0 || n_boxes < 0 || max_gt < 0 || max_ignore < 0) return MR_ERR_BAD_ARGUMENT;
    if (box_stride != 4 && box_stride != 5) return MR_ERR_BAD_ARGUMENT;
    if (image_stride < 0 || (image_stride > 0 && image_stride < (int64_t)n_boxes * box_stride)) return MR_ERR_BAD_ARGUMENT;
    if (!means || !stds) return MR_ERR_BAD_ARGUMENT;
    if (max_gt > kAssignMaxGt || max_ignore > kAssignMaxIgnore || n_images > kAssignMaxImages) return MR_ERR_UNSUPPORTED;
    if ((long long)n_images * n_boxes > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    if (n_images == 0 || n_boxes == 0) return MR_OK;
    if (!boxes || !gt_offsets || !max_overlap || !argmax || !ignored || !gt_ind) return MR_ERR_BAD_ARGUMENT;
    if (max_gt > 0 && (!gt_bboxes || !workspace)) return MR_ERR_BAD_ARGUMENT;
    if (max_ignore > 0 && (!ignore_bboxes != !ignore_offsets)) return MR_ERR_BAD_ARGUMENT;
    AssignArgs a;
    memset(&a, 0, sizeof a);
    a.boxes = boxes; a.image_stride = image_stride; a.box_stride = box_stride; a.valid = valid; a.counts = (const int *)counts;
    a.N = n_images; a.B = n_boxes;
    a.gt = gt_bboxes; a.gt_offsets = (const int *)gt_offsets; a.gt_labels = (const int *)gt_labels; a.max_gt = max_gt;
    const bool with_ignore = max_ignore > 0 && ignore_bboxes && ignore_offsets;
    a.ign = with_ignore ? ignore_bboxes : nullptr; a.ign_offsets = with_ignore ? (const int *)ignore_offsets : nullptr;
    a.max_ign = with_ignore ? max_ignore : 0;
    a.pos_thr = pos_iou_thr; a.neg_thr = neg_iou_thr; a.min_pos = min_pos_iou; a.ign_thr = ignore_iof_thr;
    a.low_quality = match_low_quality != 0;
    for (int k = 0; k < 4; ++k) { a.mean[k] = means[k]; a.std[k] = stds[k]; }
    a.max_overlap = max_overlap; a.argmax = (int *)argmax; a.ignored = ignored; a.gt_max = gt_max; a.gt_ind = (int *)gt_ind;
    a.label = (int *)label; a.deltas = deltas; a.keys = (unsigned *)workspace;
    if (max_gt > 0) HIP_TRY(hipMemsetAsync(workspace, 0, mr_assign_workspace_bytes(n_images, max_gt), (hipStream_t)stream));
    const dim3 grid((unsigned)((n_boxes + kAssignThreads - 1) / kAssignThreads), (unsigned)n_images);
    hipLaunchKernelGGL(assign_max_kernel, grid, dim3(kAssignThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(assign_finish_kernel, grid, dim3(kAssignThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
