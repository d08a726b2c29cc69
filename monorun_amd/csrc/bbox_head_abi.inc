// include/monorun_bbox.h: the 2-D detection head's get_bboxes (mmdet's Shared2FCBBoxHead: softmax, delta2bbox per class, multiclass_nms)
static int bbox_check_sizes(int n_rois, int n_images, int num_classes, int max_rois) {
    static_assert(kBboxMaxRois == MR_BBOX_MAX_ROIS && kBboxMaxRois == kNmsMaxGroup && kBboxMaxClasses == MR_BBOX_MAX_CLASSES,
                  "the header states the caps");
    static_assert(sizeof(unsigned long long) * kBboxMaxRois == MR_BBOX_RANK_LDS_BYTES, "the header states the LDS");
    static_assert((sizeof(unsigned long long) + sizeof(int)) * kBboxMaxClasses * kBboxWords == MR_BBOX_SELECT_LDS_BYTES, "the header states the LDS");
    if (n_rois < 0 || n_images < 0 || num_classes < 1 || max_rois < 0) return MR_ERR_BAD_ARGUMENT;
    if (max_rois > kBboxMaxRois || num_classes > kBboxMaxClasses || n_images > MR_BBOX_MAX_IMAGES) return MR_ERR_UNSUPPORTED;
    if ((long long)n_rois * num_classes * 4 > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    return MR_OK;
}

int mr_bbox_head_rank(const float *cls_score, const float *bbox_pred, const float *rois, const int32_t *row_offsets, const float *img_shape,
                      const float *scale_factor, int n_rois, int n_images, int num_classes, int reg_class_agnostic, int max_rois,
                      const float *means, const float *stds, double wh_ratio_clip, float score_thr, float *boxes, float *score,
                      int32_t *order, uint8_t *valid, int32_t *group_offsets, void *stream) {
    const int bad = bbox_check_sizes(n_rois, n_images, num_classes, max_rois);
    if (bad) return bad;
    if (!means || !stds || !(wh_ratio_clip > 0.0) || !(fabs(log(wh_ratio_clip)) < 1e30)) return MR_ERR_BAD_ARGUMENT;
    if (n_rois == 0 || n_images == 0 || max_rois == 0) return MR_OK;
    if (!cls_score || !bbox_pred || !rois || !row_offsets || !img_shape || !boxes || !score || !order || !valid || !group_offsets)
        return MR_ERR_BAD_ARGUMENT;
    BboxRankArgs a;
    memset(&a, 0, sizeof a);
    a.cls = cls_score; a.reg = bbox_pred; a.rois = rois; a.row_offsets = (const int *)row_offsets; a.img_shape = img_shape; a.scale = scale_factor;
    a.R = n_rois; a.N = n_images; a.C = num_classes; a.agnostic = reg_class_agnostic ? 1 : 0; a.max_rois = max_rois;
    for (int k = 0; k < 4; ++k) { a.mean[k] = means[k]; a.std[k] = stds[k]; }
    a.max_ratio = (float)fabs(log(wh_ratio_clip)); a.score_thr = score_thr;
    a.boxes = boxes; a.score = score; a.order = (int *)order; a.valid = valid; a.group_offsets = (int *)group_offsets;
    hipLaunchKernelGGL(bbox_head_rank_kernel, dim3((unsigned)num_classes, (unsigned)n_images), dim3(kBboxThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_bbox_head_select(const float *boxes, const float *score, const int32_t *order, const uint8_t *keep, const int32_t *row_offsets,
                        int n_rois, int n_images, int num_classes, int max_rois, int max_num, float *dets, int64_t *labels, int32_t *counts,
                        void *stream) {
    const int bad = bbox_check_sizes(n_rois, n_images, num_classes, max_rois);
    if (bad) return bad;
    if (max_num < 1) return MR_ERR_BAD_ARGUMENT;
    if ((long long)n_images * max_num * 5 > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    if (n_rois == 0 || n_images == 0 || max_rois == 0) return MR_OK;
    if (!boxes || !score || !order || !keep || !row_offsets || !dets || !labels || !counts) return MR_ERR_BAD_ARGUMENT;
    BboxSelectArgs a;
    memset(&a, 0, sizeof a);
    a.boxes = boxes; a.score = score; a.order = (const int *)order; a.keep = keep; a.row_offsets = (const int *)row_offsets;
    a.R = n_rois; a.N = n_images; a.C = num_classes; a.max_rois = max_rois; a.max_num = max_num;
    a.dets = dets; a.labels = (long long *)labels; a.counts = (int *)counts;
    hipLaunchKernelGGL(bbox_head_select_kernel, dim3((unsigned)n_images), dim3(kBboxThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// The workspace of mr_bbox_head_detect, T = n_rois num_classes candidates: the NMS's bit matrix (bounded from above: every group has at
// most min(n_rois, max_rois) boxes), boxes, score, order, the group offsets, the groups' kept counts, valid and keep.
static size_t bbox_nms_words(int n_rois, int num_classes, int max_rois) {
    const size_t g = (size_t)(n_rois < max_rois ? n_rois : max_rois);
    return (size_t)n_rois * num_classes * ((g + kNmsTile - 1) / kNmsTile);
}

size_t mr_bbox_head_workspace_bytes(int n_rois, int n_images, int num_classes, int max_rois) {
    if (n_rois < 0 || n_images < 0 || num_classes < 1 || max_rois < 0) return 0;
    const size_t T = (size_t)n_rois * num_classes, G = (size_t)n_images * num_classes;
    return 8 * bbox_nms_words(n_rois, num_classes, max_rois) + T * (16 + 4 + 4) + (2 * G + 2) * 4 + 2 * T + 8;
}

int mr_bbox_head_detect(const float *cls_score, const float *bbox_pred, const float *rois, const int32_t *row_offsets, const float *img_shape,
                        const float *scale_factor, int n_rois, int n_images, int num_classes, int reg_class_agnostic, int max_rois,
                        const float *means, const float *stds, double wh_ratio_clip, float score_thr, float iou_thr, int max_num,
                        float *dets, int64_t *labels, int32_t *counts, void *workspace, void *stream) {
    const int bad = bbox_check_sizes(n_rois, n_images, num_classes, max_rois);
    if (bad) return bad;
    if (max_num < 1 || !means || !stds || !(wh_ratio_clip > 0.0) || !(fabs(log(wh_ratio_clip)) < 1e30)) return MR_ERR_BAD_ARGUMENT;
    if ((long long)n_images * max_num * 5 > 0x7fffffffLL || (long long)n_images * num_classes > kNmsMaxGroups) return MR_ERR_UNSUPPORTED;
    if (n_rois == 0 || n_images == 0 || max_rois == 0) return MR_OK;
    if (!cls_score || !bbox_pred || !rois || !row_offsets || !img_shape || !dets || !labels || !counts || !workspace) return MR_ERR_BAD_ARGUMENT;
    const size_t T = (size_t)n_rois * num_classes, G = (size_t)n_images * num_classes;
    unsigned long long *matrix = (unsigned long long *)workspace;
    float *boxes = (float *)(matrix + bbox_nms_words(n_rois, num_classes, max_rois));
    float *score = boxes + 4 * T;
    int32_t *order = (int32_t *)(score + T), *group_offsets = order + T, *num_keep = group_offsets + G + 1;
    uint8_t *valid = (uint8_t *)(num_keep + G + 1), *keep = valid + T;
    int code = mr_bbox_head_rank(cls_score, bbox_pred, rois, row_offsets, img_shape, scale_factor, n_rois, n_images, num_classes,
                                 reg_class_agnostic, max_rois, means, stds, wh_ratio_clip, score_thr, boxes, score, order, valid, group_offsets,
                                 stream);
    if (code) return code;
    code = mr_nms_grouped(boxes, valid, group_offsets, (int)G, n_rois < max_rois ? n_rois : max_rois, iou_thr, keep, num_keep, matrix, stream);
    if (code) return code;
    return mr_bbox_head_select(boxes, score, order, keep, row_offsets, n_rois, n_images, num_classes, max_rois, max_num, dets, labels, counts,
                               stream);
}
