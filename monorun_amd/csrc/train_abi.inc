// include/monorun_train.h: the NOC head's training decode, forward and backward (monorun_roi_head.py:189-217, :374-394).
// fill_decode_args: pnp_decode_abi.inc.
static int fill_decode_train_args(DecodeTrainArgs &t, const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                                  const float *dim_var, int n, int num_classes, int class_agnostic, int h, int w,
                                  const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                                  double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain) {
    memset(&t, 0, sizeof t);
    const int rc = fill_decode_args(t.d, all_pred, pred_dtype, labels, flip, dim, dim_var, nullptr, n, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                    noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain, 1.0f, -1.0f, false);
    if (rc != MR_OK) return rc;
    if ((long long)h * w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    t.sdf = (float)proj_scaling_denominator;
    return MR_OK;
}

int mr_noc_decode_train(const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                        const float *dim_var, const float *distances, int n, int num_classes, int class_agnostic, int h, int w,
                        const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                        double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, double distance_min,
                        float *noc_pred, float *proj_logstd, float *coords_3d, float *coords_3d_var, float *proj_logstd_px,
                        float *dims, float *dims_var, void *stream) {
    if (n == 0) return MR_OK;
    DecodeTrainArgs t;
    const int rc = fill_decode_train_args(t, all_pred, pred_dtype, labels, flip, dim, dim_var, n, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                          noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain);
    if (rc != MR_OK) return rc;
    if (!noc_pred || !proj_logstd || !coords_3d || !proj_logstd_px || !dims || (dim_var && (!coords_3d_var || !dims_var))) return MR_ERR_BAD_ARGUMENT;
    t.distances = distances; t.dist_min = (float)distance_min;
    t.noc = noc_pred; t.ls = proj_logstd; t.d.c3d = coords_3d; t.c3d_var = coords_3d_var; t.lspx = proj_logstd_px; t.d.dims = dims; t.d.dims_var = dims_var;
    return launch_noc_decode_train(t, (hipStream_t)stream);
}

int mr_noc_decode_train_backward(const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                                 const float *dim_var, int n, int num_classes, int class_agnostic, int h, int w,
                                 const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                                 double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain,
                                 const float *grad_noc_pred, const float *grad_proj_logstd, const float *grad_coords_3d,
                                 const float *grad_coords_3d_var, const float *grad_proj_logstd_px, const float *grad_dims,
                                 const float *grad_dims_var, void *grad_all_pred, float *grad_dim, float *grad_dim_var, void *stream) {
    if (n == 0) return MR_OK;
    DecodeTrainArgs t;
    const int rc = fill_decode_train_args(t, all_pred, pred_dtype, labels, flip, dim, dim_var, n, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                          noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain);
    if (rc != MR_OK) return rc;
    if (!grad_all_pred || !grad_dim || (dim_var && !grad_dim_var)) return MR_ERR_BAD_ARGUMENT;
    t.g_noc = grad_noc_pred; t.g_ls = grad_proj_logstd; t.g_c3d = grad_coords_3d; t.g_c3d_var = grad_coords_3d_var; t.g_lspx = grad_proj_logstd_px;
    t.g_dims = grad_dims; t.g_dims_var = grad_dims_var;
    t.grad_all_pred = grad_all_pred; t.grad_dim = grad_dim; t.grad_dim_var = grad_dim_var;
    return launch_noc_decode_train_backward(t, (hipStream_t)stream);
}
