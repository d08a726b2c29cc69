// include/monorun_pnp.h, the training losses.
// ---- the aligned rotated 3-D IoU of the pose head's loss (bbox3d_iou_calculator.py:166-192)
int mr_bbox3d_overlaps_aligned(const float *boxes, int64_t boxes_row_stride, const float *qboxes, int64_t qboxes_row_stride, int n,
                               int criterion, int z_axis, float z_center, int flags, float *iou, float *rinc, void *stream) {
    if (n < 0 || criterion < -1 || criterion > 2 || z_axis < 0 || z_axis > 2 || (flags & ~MR_IOU3D_GEOMETRIC_HEIGHT)) return MR_ERR_BAD_ARGUMENT;
    if (boxes_row_stride < 7 || qboxes_row_stride < 7) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!boxes || !qboxes || !iou) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(bbox3d_overlaps_aligned_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                       (long long)boxes_row_stride, qboxes, (long long)qboxes_row_stride, n, criterion, z_axis, z_center,
                       (flags & MR_IOU3D_GEOMETRIC_HEIGHT) ? 1 : 0, iou, rinc);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// ---- the NOC head's training loss (uncert_projection_head.py:36-79, robust_kl_loss.py:6-30)
static int proj_check(const float *c3d, const float *pose, int64_t pose_stride, const float *K, const float *img, int n, int hw,
                      const void *out, unsigned &blocks) {
    if (n < 0 || hw < 1 || pose_stride < 4) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!c3d || !pose || !K || !img || !out) return MR_ERR_BAD_ARGUMENT;
    return grid_1d((long long)n * hw, 256, blocks) != MR_OK ? MR_ERR_UNSUPPORTED : 1;
}

int mr_uncert_projection(const float *coords_3d, const float *pose, int64_t pose_row_stride, const float *cam_intrinsic,
                         const float *img_shapes, int n, int hw, float z_min, float allowed_border, float *coords_2d, void *stream) {
    unsigned blocks;
    const int r = proj_check(coords_3d, pose, pose_row_stride, cam_intrinsic, img_shapes, n, hw, coords_2d, blocks);
    if (r != 1) return r;
    hipLaunchKernelGGL(uncert_projection_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, coords_3d, pose,
                       (long long)pose_row_stride, cam_intrinsic, img_shapes, (long long)n * hw, hw, z_min, allowed_border, coords_2d);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_uncert_projection_backward(const float *coords_3d, const float *pose, int64_t pose_row_stride, const float *cam_intrinsic,
                                  const float *img_shapes, int n, int hw, float z_min, float allowed_border, const float *grad_coords_2d,
                                  float *grad_coords_3d, void *stream) {
    unsigned blocks;
    const int r = proj_check(coords_3d, pose, pose_row_stride, cam_intrinsic, img_shapes, n, hw, grad_coords_3d, blocks);
    if (r != 1) return r;
    if (!grad_coords_2d) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(uncert_projection_backward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, coords_3d,
                       pose, (long long)pose_row_stride, cam_intrinsic, img_shapes, (long long)n * hw, hw, z_min, allowed_border, grad_coords_2d, grad_coords_3d);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int64_t mr_robust_kl_workspace_bytes(int64_t numel) {
    if (numel <= 0) return 0;
    return ((int64_t)robust_kl_blocks(numel) * 2 * (int64_t)sizeof(double) + 255) / 256 * 256;
}

// the scalars as torch rounds them: a Python float meets an fp32 tensor as fp32; (0.5 * delta) and (1 / eps) are Python arithmetic
static KlParams kl_params(int target_mode, double delta, double eps) {
    KlParams p;
    p.identity = target_mode == -1;
    p.delta = (float)delta;
    p.half_delta = (float)(0.5 * delta);
    p.inv_max = (float)(1.0 / eps);
    return p;
}

int mr_robust_kl_loss(const float *pred, const float *logstd, int64_t numel, int target_mode, double delta, double eps, double momentum,
                      int training, int reduction, double loss_weight, float *mean_inv_std, float *loss, float *c_out, void *workspace,
                      int64_t workspace_bytes, void *stream) {
    if (numel < 1 || (target_mode != 0 && target_mode != -1) || (reduction != 0 && reduction != 1) || !(eps > 0.0)) return MR_ERR_BAD_ARGUMENT;
    if (!pred || !logstd || !mean_inv_std || !loss || !c_out || !workspace) return MR_ERR_BAD_ARGUMENT;
    if (workspace_bytes < mr_robust_kl_workspace_bytes(numel)) return MR_ERR_BAD_ARGUMENT;
    const KlParams p = kl_params(target_mode, delta, eps);
    const int blocks = robust_kl_blocks(numel);
    hipLaunchKernelGGL(robust_kl_partial_kernel, dim3(blocks), dim3(kKlThreads), 0, (hipStream_t)stream, pred, logstd, (long long)numel, p,
                       (double *)workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(robust_kl_fold_kernel, dim3(1), dim3(kKlThreads), 0, (hipStream_t)stream, (const double *)workspace, blocks,
                       (long long)numel, training ? 1 : 0, (float)(1.0 - momentum), (float)momentum, reduction == 0 ? 1 : 0, (float)loss_weight,
                       mean_inv_std, loss, c_out);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_robust_kl_loss_backward(const float *pred, const float *logstd, int64_t numel, int target_mode, double delta, double eps,
                               int reduction, double loss_weight, const float *grad_loss, const float *c, float *grad_pred,
                               float *grad_logstd, void *stream) {
    if (numel < 1 || (target_mode != 0 && target_mode != -1) || (reduction != 0 && reduction != 1) || !(eps > 0.0)) return MR_ERR_BAD_ARGUMENT;
    if (!pred || !logstd || !grad_loss || !c || !grad_pred || !grad_logstd) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d(numel, kKlThreads, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(robust_kl_backward_kernel, dim3(blocks), dim3(kKlThreads), 0,
                       (hipStream_t)stream, pred, logstd, (long long)numel, kl_params(target_mode, delta, eps), grad_loss, c,
                       (float)loss_weight, reduction == 0 ? 1 : 0, grad_pred, grad_logstd);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
