// include/monorun_pnp.h, the head decode and the pose consumers: K2 (monorun_roi_head.py:189-217, :521-523), the fused decode + PnP,
// RoIAlign (mmcv.ops.roi_align) and the rotated-BEV NMS (monorun_roi_head.py:619-655).  fill_decode_args also serves train_abi.inc.
static int fill_decode_args(DecodeArgs &a, const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                            const float *dim_var, const float *rois, int B, int num_classes, int class_agnostic, int h, int w,
                            const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                            double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, float std_scale,
                            float ransac_thres_ratio, bool with_rois = true) {
    if (B < 0 || h < 1 || w < 1 || num_classes < 1) return MR_ERR_BAD_ARGUMENT;
    if (!all_pred || !labels || !flip || !dim || (with_rois && !rois) || !dim_means || !dim_stds || !noc_means || !noc_stds) return MR_ERR_BAD_ARGUMENT;
    memset(&a, 0, sizeof a);
    if (pred_dtype != MR_F32 && pred_dtype != MR_F16 && pred_dtype != MR_BF16) return MR_ERR_UNSUPPORTED;
    a.all_pred = all_pred; a.pred_dtype = pred_dtype; a.labels = (const long long *)labels; a.flip = flip; a.dim = dim; a.dim_var = dim_var; a.rois = rois;
    a.B = B; a.C = num_classes; a.agnostic = class_agnostic; a.h = h; a.w = w;
    a.dim_means = dim_means; a.dim_stds = dim_stds;
    a.noc_means = noc_means; a.noc_stds = noc_stds;
    // python-scalar constants of distance_invar_proj_error_coder.py:50-54, rounded the way torch rounds them
    const double e = ref_focal_y * epistemic_std_gain;
    a.k_epi = (float)(e * e);
    a.k_sd2 = (float)(proj_scaling_denominator * proj_scaling_denominator);
    const float sdf = (float)proj_scaling_denominator;
    a.sd_sq = sdf * sdf;
    a.std_scale = std_scale; a.ratio = ransac_thres_ratio; a.has_var = dim_var != nullptr;
    a.w_magic = (w > 1 && (long long)h * w < 65536) ? 0xFFFFFFFFu / (unsigned)w + 1u : 0u;
    return MR_OK;
}

int mr_noc_decode_batched(
    const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim, const float *dim_var, const float *rois,
    int B, int num_classes, int class_agnostic, int h, int w,
    const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
    double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, float std_scale, float ransac_thres_ratio,
    float *coords_2d, float *coords_2d_istd, float *coords_3d, float *dims, float *dims_var, float *ransac_thr,
    const float *coord_2d_map, int map_h, int map_w, void *stream) {
    if (B == 0) return MR_OK;
    if (coord_2d_map && (map_h < 1 || map_w < 1)) return MR_ERR_BAD_ARGUMENT;
    DecodeArgs a;
    const int rc = fill_decode_args(a, all_pred, pred_dtype, labels, flip, dim, dim_var, rois, B, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                    noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain, std_scale, ransac_thres_ratio);
    if (rc != MR_OK) return rc;
    if (!coords_2d || !coords_2d_istd || !coords_3d) return MR_ERR_BAD_ARGUMENT;
    a.c2d = coords_2d; a.istd = coords_2d_istd; a.c3d = coords_3d; a.dims = dims; a.dims_var = dims_var;
    a.thr = (ransac_thres_ratio >= 0.f) ? ransac_thr : nullptr;
    a.map2d = coord_2d_map; a.map_h = map_h; a.map_w = map_w;
    const int hw = h * w;
    const bool x4 = pred_dtype == MR_F32 && !coord_2d_map && (hw % 4 == 0) && a.w_magic != 0u &&      // w_magic: p / w by multiplication (decode_pixel_pair)
                    ((((uintptr_t)all_pred | (uintptr_t)coords_2d | (uintptr_t)coords_2d_istd | (uintptr_t)coords_3d) & 15) == 0);
    if (x4) {
        // 256 threads x one quad measured best (13.1 us per 1024 x 28x28 batch; 128 x 2 quads 14.2, 64 x 4 quads 25.5: the kernel wants threads, not trips);
        // a persistent, three-stage software-pipelined form (loads of the next quad in flight during the arithmetic; bit-identical outputs) is NOT faster:
        // 13.0 - 14.9 us against 12.5 in the same session (profiles/r04_k2_pipelined_experiment.txt)
        hipLaunchKernelGGL((noc_decode_kernel_x4<256, 1>), dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a, hw / 4);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    }
    unsigned blocks;
    if (grid_1d((long long)((hw + 255) / 256) * B, 1, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;      // (hw + 255) / 256 workgroups per object
    hipLaunchKernelGGL(noc_decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_pnp_from_head_batched(
    const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim, const float *dim_var, const float *rois,
    int B, int num_classes, int class_agnostic, int h, int w,
    const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
    double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, float std_scale, float ransac_thres_ratio,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    float z_min, float istd_thres, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag,
    float *dims, float *dims_var, const float *coord_2d_map, int map_h, int map_w,
    const float *cov_calib_logscale, float cov_corr_sd, float *cov_calib, void *stream) {
    const int P = h * w;
    if (B < 0 || P < 4 || P > 64 * kMaxChunks) return MR_ERR_BAD_ARGUMENT;
    if (coord_2d_map && (map_h < 1 || map_w < 1)) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!cam_mats || !u_range || !v_range || !valid || !pose || !tr_radius || (!cov && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    // the tile is built channel-planar, exactly the layout (and hence numpy summation order) the reference's head produces
    const int64_t s2[3] = { 2LL * P, 1, P }, s3[3] = { 3LL * P, 1, P };
    const CorrIn in{ nullptr, s2, nullptr, s2, nullptr, s3, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    PnpArgs a;
    memset(&a, 0, sizeof a);
    const int rc = fill_decode_args(a.dec, all_pred, pred_dtype, labels, flip, dim, dim_var, rois, B, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                    noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain, std_scale, ransac_thres_ratio);
    if (rc != MR_OK) return rc;
    a.dec.dims = dims; a.dec.dims_var = dims_var;
    a.dec.map2d = coord_2d_map; a.dec.map_h = map_h; a.dec.map_w = map_w;
    if (cov_calib && (!cov_calib_logscale || (flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    a.calib_logscale = cov_calib_logscale; a.corr_sd = cov_corr_sd; a.cov_calib = cov_calib;
    a.from_head = 1;
    set_inputs(a, in);
    a.B = B; a.P = P; a.z_min = (double)z_min; a.istd_thres = istd_thres; a.inlier_opt_only = inlier_opt_only; a.flags = flags;
    a.valid = valid; a.pose = pose; a.cov = cov; a.tr = tr_radius; a.mask = inlier_mask; a.diag = diag;
    a.stamps = g_stamps;
    int r;
    if ((r = choose_mean_order(a)) != MR_OK) return r;
    return launch_wpo<float>(a, lm_launch_waves(a, flags, MR_F32), (hipStream_t)stream);
}

int mr_roi_align_avg(const float *input, const float *rois, int K, int C, int H, int W, int out_h, int out_w,
                     float spatial_scale, int sampling_ratio, int aligned, float *output, void *stream) {
    if (K < 0 || C < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) return MR_ERR_BAD_ARGUMENT;
    if (K == 0) return MR_OK;
    if (!input || !rois || !output) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d((long long)K * C * out_h * out_w, 256, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(roi_align_avg_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, input, rois, K, C, H, W, out_h, out_w,
                       spatial_scale, sampling_ratio, aligned, output);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_nms_bev_batched(const float *boxes_xyxyr, const float *scores, const int32_t *offsets, int groups, int max_group,
                       float thr, int64_t *keep, int32_t *num_keep, void *stream) {
    if (groups < 0 || max_group < 0) return MR_ERR_BAD_ARGUMENT;
    if (groups == 0) return MR_OK;
    if (!offsets || !keep || !num_keep || (max_group > 0 && (!boxes_xyxyr || !scores))) return MR_ERR_BAD_ARGUMENT;
    if (max_group > kNmsMax) return MR_ERR_UNSUPPORTED;
    int np2 = 1; while (np2 < max_group) np2 <<= 1;
    const size_t lds = (size_t)np2 * 8 + (size_t)max_group * sizeof(NmsBox) + (size_t)max_group * ((max_group + 31) / 32) * 4 + 16;
    hipLaunchKernelGGL(nms_bev_kernel, dim3(groups), dim3(256), lds, (hipStream_t)stream, boxes_xyxyr, scores, (const int *)offsets, thr,
                       (long long *)keep, (int *)num_keep);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
