// include/monorun_roi.h: the multi-level RoI feature extractor, SingleRoIExtractor over RoIAlign (mmdet / mmcv.ops.roi_align)
static int roi_extract_fill(RoiExtractArgs &a, float *const *maps, const int *level_h, const int *level_w, const int *level_stride, int n_levels,
                            int n_images, int channels, const float *rois, const float *level_rois, int n_rois, float finest_scale, int out_h,
                            int out_w, int sampling_ratio, int aligned, bool backward, long long &blocks) {
    static_assert(kRoiMaxLevels == MR_ROI_MAX_LEVELS && kRoiMaxOut == MR_ROI_MAX_OUT && kRoiChunk == MR_ROI_CHUNK && kRoiTaps == MR_ROI_TAPS &&
                  kRoiTileH == MR_ROI_TILE_H && kRoiTileW == MR_ROI_TILE_W && kRoiBwdChunk == MR_ROI_BWD_CHUNK, "the header states the tiling");
    static_assert(sizeof(RoiTapLds) * 2 * kRoiTaps == MR_ROI_FORWARD_LDS_BYTES && sizeof(RoiBwdLds) == MR_ROI_BACKWARD_LDS_BYTES,
                  "the header states the LDS");
    if (n_levels < 1 || n_images < 1 || channels < 1 || out_h < 1 || out_w < 1 || n_rois < 0 || sampling_ratio < 0 || !(finest_scale > 0.0f))
        return MR_ERR_BAD_ARGUMENT;
    if (!maps || !level_h || !level_w || !level_stride) return MR_ERR_BAD_ARGUMENT;
    if (n_levels > kRoiMaxLevels || out_h > kRoiMaxOut || out_w > kRoiMaxOut) return MR_ERR_UNSUPPORTED;
    if ((long long)n_rois * channels * out_h * out_w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    memset(&a, 0, sizeof a);
    blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (level_h[l] < 1 || level_w[l] < 1 || level_stride[l] < 1 || !maps[l]) return MR_ERR_BAD_ARGUMENT;
        if ((long long)channels * level_h[l] * level_w[l] > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
        if (backward && blocks > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;      // the tile grid is the backward's alone
        a.lv[l] = RoiLevel{ maps[l], level_h[l], level_w[l], level_stride[l], (unsigned)blocks };
        blocks += (long long)n_images * ((channels + kRoiBwdChunk - 1) / kRoiBwdChunk) * ((level_h[l] + kRoiTileH - 1) / kRoiTileH) *
                  ((level_w[l] + kRoiTileW - 1) / kRoiTileW);
    }
    if (!backward) blocks = (long long)n_rois * ((channels + kRoiChunk - 1) / kRoiChunk);
    if (blocks > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    a.rois = rois; a.level_rois = level_rois ? level_rois : rois; a.L = n_levels; a.N = n_images; a.C = channels; a.K = n_rois; a.oh = out_h; a.ow = out_w;
    a.sampling_ratio = sampling_ratio; a.aligned = aligned ? 1 : 0; a.finest_scale = finest_scale;
    return MR_OK;
}

int mr_roi_extract_forward(const float *const *feats, const int *level_h, const int *level_w, const int *level_stride, int n_levels,
                           int n_images, int channels, const float *rois, const float *level_rois, int n_rois, float finest_scale,
                           int out_h, int out_w, int sampling_ratio, int aligned, float *out, void *stream) {
    RoiExtractArgs a;
    long long blocks;
    const int rc = roi_extract_fill(a, (float *const *)feats, level_h, level_w, level_stride, n_levels, n_images, channels, rois, level_rois,
                                    n_rois, finest_scale, out_h, out_w, sampling_ratio, aligned, false, blocks);
    if (rc != MR_OK) return rc;
    if (n_rois == 0) return MR_OK;
    if (!rois || !out) return MR_ERR_BAD_ARGUMENT;
    a.out = out;
    hipLaunchKernelGGL(roi_extract_forward_kernel, dim3((unsigned)blocks), dim3(kRoiThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_roi_extract_backward(const float *grad_out, const float *rois, const float *level_rois, int n_rois, float *const *grad_feats,
                            const int *level_h, const int *level_w, const int *level_stride, int n_levels, int n_images, int channels,
                            float finest_scale, int out_h, int out_w, int sampling_ratio, int aligned, void *stream) {
    RoiExtractArgs a;
    long long blocks;
    const int rc = roi_extract_fill(a, grad_feats, level_h, level_w, level_stride, n_levels, n_images, channels, rois, level_rois, n_rois,
                                    finest_scale, out_h, out_w, sampling_ratio, aligned, true, blocks);
    if (rc != MR_OK) return rc;
    if (n_rois > 0 && (!rois || !grad_out)) return MR_ERR_BAD_ARGUMENT;
    a.out = (float *)grad_out;          // read only by this kernel
    hipLaunchKernelGGL(roi_extract_backward_kernel, dim3((unsigned)blocks), dim3(kRoiThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
