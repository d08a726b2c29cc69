// include/monorun_proposals.h: the proposal stage, mmdet's RPNHead.get_bboxes (delta2bbox) and mmcv's nms / batched_nms
int mr_proposal_decode(const float *const *cls, const float *const *reg, const int *level_h, const int *level_w, const int *level_stride,
                       const int *level_count, const float *base_anchors, int n_levels, int n_anchors, int n_images, const int64_t *index,
                       const float *img_shape, const float *means, const float *stds, double wh_ratio_clip, float min_bbox_size,
                       float *boxes, float *score, float *logit, uint8_t *valid, void *stream) {
    static_assert(kPropMaxLevels == MR_PROPOSAL_MAX_LEVELS && kPropMaxAnchors == MR_PROPOSAL_MAX_ANCHORS, "the header states the caps");
    static_assert(sizeof(ProposalArgs) <= 4096, "the level table fits the kernel arguments");
    if (n_levels < 1 || n_images < 1 || n_anchors < 1) return MR_ERR_BAD_ARGUMENT;
    if (!cls || !reg || !level_h || !level_w || !level_stride || !level_count || !base_anchors || !means || !stds) return MR_ERR_BAD_ARGUMENT;
    if (!(wh_ratio_clip > 0.0) || !(fabs(log(wh_ratio_clip)) < 1e30)) return MR_ERR_BAD_ARGUMENT;
    if (n_levels > kPropMaxLevels || n_anchors > kPropMaxAnchors) return MR_ERR_UNSUPPORTED;
    if ((long long)n_images * n_levels > 65535) return MR_ERR_UNSUPPORTED;
    ProposalArgs a;
    memset(&a, 0, sizeof a);
    long long per_image = 0;
    int max_count = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (level_h[l] < 1 || level_w[l] < 1 || level_stride[l] < 1 || level_count[l] < 0 || !cls[l] || !reg[l]) return MR_ERR_BAD_ARGUMENT;
        if ((long long)n_images * 4 * n_anchors * level_h[l] * level_w[l] > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
        ProposalLevel &lv = a.lv[l];
        lv.cls = cls[l]; lv.reg = reg[l]; lv.H = level_h[l]; lv.W = level_w[l]; lv.stride = level_stride[l];
        lv.count = level_count[l]; lv.first = (int)per_image;
        for (int k = 0; k < n_anchors * 4; ++k) lv.base[k / 4][k % 4] = base_anchors[((size_t)l * n_anchors) * 4 + k];
        per_image += level_count[l];
        if (per_image * n_images > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
        if (level_count[l] > max_count) max_count = level_count[l];
    }
    if (per_image == 0) return MR_OK;
    if (!index || !img_shape || !boxes || !score || !logit || !valid) return MR_ERR_BAD_ARGUMENT;
    a.index = (const long long *)index; a.img_shape = img_shape;
    for (int k = 0; k < 4; ++k) { a.mean[k] = means[k]; a.std[k] = stds[k]; }
    a.max_ratio = (float)fabs(log(wh_ratio_clip)); a.min_size = min_bbox_size;
    a.L = n_levels; a.N = n_images; a.A = n_anchors; a.per_image = (int)per_image;
    a.boxes = boxes; a.score = score; a.logit = logit; a.valid = valid;
    const dim3 grid((unsigned)((max_count + kPropThreads - 1) / kPropThreads), (unsigned)(n_images * n_levels));
    hipLaunchKernelGGL(proposal_decode_kernel, grid, dim3(kPropThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

size_t mr_nms_workspace_bytes(const int *group_sizes, int groups, int max_group) {
    if (!group_sizes || groups < 0 || max_group < 0) return 0;
    size_t words = 0;
    for (int g = 0; g < groups; ++g) {
        const size_t n = (size_t)(group_sizes[g] < 0 ? 0 : group_sizes[g] > max_group ? max_group : group_sizes[g]);
        words += n * ((n + kNmsTile - 1) / kNmsTile);
    }
    return words * sizeof(unsigned long long);
}

int mr_nms_grouped(const float *boxes, const uint8_t *valid, const int32_t *offsets, int groups, int max_group, float thr,
                   uint8_t *keep, int32_t *num_keep, void *workspace, void *stream) {
    static_assert(kNmsMaxGroup == MR_NMS_MAX_GROUP && kNmsMaxGroups == MR_NMS_MAX_GROUPS && kNmsTile == MR_NMS_TILE &&
                  kNmsScanRows == MR_NMS_SCAN_ROWS && 2 * kNmsScanRows == kNmsTile, "the header states the tiling");
    static_assert(sizeof(float) * 4 * kNmsTile == MR_NMS_MASK_LDS_BYTES, "the header states the LDS");
    if (groups < 0 || max_group < 0) return MR_ERR_BAD_ARGUMENT;
    if (groups == 0 || max_group == 0) return MR_OK;
    if (!boxes || !offsets || !keep || !num_keep || !workspace) return MR_ERR_BAD_ARGUMENT;
    if (max_group > kNmsMaxGroup || groups > kNmsMaxGroups) return MR_ERR_UNSUPPORTED;
    const unsigned nb = (unsigned)((max_group + kNmsTile - 1) / kNmsTile);
    hipLaunchKernelGGL(nms_mask_kernel, dim3(nb * (nb + 1) / 2, (unsigned)groups), dim3(kNmsTile), 0, (hipStream_t)stream, boxes,
                       (const int *)offsets, max_group, thr, (unsigned long long *)workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(nms_scan_kernel, dim3((unsigned)groups), dim3(64), 0, (hipStream_t)stream, (const unsigned long long *)workspace, valid,
                       (const int *)offsets, max_group, keep, (int *)num_keep);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
