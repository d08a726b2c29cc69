// include/monorun_targets.h: the NOC head's LiDAR supervision (masked_dense_target.py, noc_coder.py:17-48, smooth_l1_loss.py)
int mr_noc_dense_target(int num_images, const float *const *coords_3d, const float *const *coords_3d_mask, const float *const *dimensions,
                        const int64_t *dimensions_row_stride, const int32_t *map_h, const int32_t *map_w, const int32_t *num_gt,
                        const uint8_t *flip, const float *rois, const int32_t *roi_img, const int64_t *roi_gt, int n, int h, int w,
                        const float *target_means, const float *target_stds, double eps_coder, double eps_target,
                        float *targets, float *weights, int32_t *counts, void *stream) {
    if (n < 0 || num_images < 0 || h < 1 || w < 1) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!rois || !roi_img || !roi_gt || !target_means || !target_stds || !targets || !weights || !counts) return MR_ERR_BAD_ARGUMENT;
    if (num_images > 0 && (!coords_3d || !coords_3d_mask || !dimensions || !dimensions_row_stride || !map_h || !map_w || !num_gt || !flip))
        return MR_ERR_BAD_ARGUMENT;
    if (num_images > kNocMaxImages || (long long)n * h * w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    NocTargetArgs a;
    memset(&a, 0, sizeof a);
    for (int j = 0; j < num_images; ++j) {
        if (map_h[j] < 1 || map_w[j] < 1 || num_gt[j] < 0) return MR_ERR_BAD_ARGUMENT;
        if (num_gt[j] > 0 && (!coords_3d[j] || !coords_3d_mask[j] || !dimensions[j] || dimensions_row_stride[j] < 3)) return MR_ERR_BAD_ARGUMENT;
        NocImage &im = a.img[j];
        im.coords = coords_3d[j]; im.mask = coords_3d_mask[j]; im.dims = dimensions[j]; im.dims_stride = (long long)dimensions_row_stride[j];
        im.H = map_h[j]; im.W = map_w[j]; im.G = num_gt[j]; im.flip = flip[j] ? 1 : 0;
    }
    a.num_images = num_images;
    a.rois = rois; a.roi_img = (const int *)roi_img; a.roi_gt = (const long long *)roi_gt;
    a.n = n; a.h = h; a.w = w;
    a.means = target_means; a.stds = target_stds;
    a.eps_c = (float)eps_coder; a.eps_t = (float)eps_target;          // a Python float meets an fp32 tensor as fp32
    a.targets = targets; a.weights = weights; a.counts = (int *)counts;
    hipLaunchKernelGGL(noc_dense_target_kernel, dim3((unsigned)n), dim3(kNocThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(noc_target_normalise_kernel, dim3((unsigned)n), dim3(kNocThreads), 0, (hipStream_t)stream, (const int *)counts, n, h * w,
                       a.eps_t, weights);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int64_t mr_smooth_l1_mod_workspace_bytes(int64_t numel) {
    if (numel <= 0) return 0;
    return ((int64_t)robust_kl_blocks(numel) * (int64_t)sizeof(double) + 255) / 256 * 256;
}

static int sl1_params(const void *pred, const void *target, const void *weight, int weight_mode, int64_t numel, int channels, int64_t hw,
                      double beta, int reduction, Sl1Params &p) {
    if (numel < 1 || !(beta > 0.0) || (reduction != 0 && reduction != 1) || weight_mode < 0 || weight_mode > 2) return MR_ERR_BAD_ARGUMENT;
    if (!pred || !target || (weight_mode != 0 && !weight)) return MR_ERR_BAD_ARGUMENT;
    p.beta = (float)beta; p.half_beta = (float)(0.5 * beta); p.weight_mode = weight_mode; p.chw = 1; p.hw = 1;
    if (weight_mode == 2) {
        if (channels < 1 || hw < 1 || numel % ((int64_t)channels * hw) != 0) return MR_ERR_BAD_ARGUMENT;
        p.chw = (long long)channels * hw; p.hw = (long long)hw;
    }
    return MR_OK;
}

int mr_smooth_l1_mod_loss(const float *pred, const float *target, const float *weight, int weight_mode, int64_t numel, int channels, int64_t hw,
                          double beta, int reduction, double loss_weight, float *loss, void *workspace, int64_t workspace_bytes, void *stream) {
    Sl1Params p;
    const int r = sl1_params(pred, target, weight, weight_mode, numel, channels, hw, beta, reduction, p);
    if (r != MR_OK) return r;
    if (!loss || !workspace || workspace_bytes < mr_smooth_l1_mod_workspace_bytes(numel)) return MR_ERR_BAD_ARGUMENT;
    const int blocks = robust_kl_blocks(numel);
    hipLaunchKernelGGL(smooth_l1_mod_loss_kernel, dim3(blocks), dim3(kKlThreads), 0, (hipStream_t)stream, pred, target, weight, (long long)numel, p,
                       (double *)workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(smooth_l1_mod_finish_kernel, dim3(1), dim3(kKlThreads), 0, (hipStream_t)stream, (const double *)workspace, blocks,
                       (long long)numel, reduction == 0 ? 1 : 0, (float)loss_weight, loss);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_smooth_l1_mod_loss_backward(const float *pred, const float *target, const float *weight, int weight_mode, int64_t numel, int channels,
                                   int64_t hw, double beta, int reduction, double loss_weight, const float *grad_loss, float *grad_pred,
                                   void *stream) {
    Sl1Params p;
    const int r = sl1_params(pred, target, weight, weight_mode, numel, channels, hw, beta, reduction, p);
    if (r != MR_OK) return r;
    if (!grad_loss || !grad_pred) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d(numel, kKlThreads, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(smooth_l1_mod_loss_backward_kernel, dim3(blocks), dim3(kKlThreads), 0, (hipStream_t)stream, pred, target, weight,
                       (long long)numel, p, grad_loss, (float)loss_weight, reduction == 0 ? 1 : 0, grad_pred);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
