// include/monorun_heads.h: the score head's eval-mode forward with its epilogue (mlp_score_head.py:94-115, monorun_roi_head.py:544-550)
int mr_score_head_forward(const float *reg_fc_out, int64_t reg_fc_out_row_stride, const float *yaw, int64_t yaw_row_stride,
                          const float *t_vec, int64_t t_vec_row_stride, const float *pose_cov, const float *dimensions,
                          int64_t dimensions_row_stride, const uint8_t *ret_val, const float *scores_2d, const float *params,
                          int64_t params_numel, int n, int c1, int c2, int flags, float *scores, void *stream) {
    if (n < 0 || c1 < 1 || c1 > MR_SCORE_MAX_C1 || c2 < 1 || c2 > MR_SCORE_MAX_C2 || (flags & ~MR_SCORE_SIGMOID)) return MR_ERR_BAD_ARGUMENT;
    if (reg_fc_out_row_stride < c1 || yaw_row_stride < 1 || t_vec_row_stride < 3 || dimensions_row_stride < 3) return MR_ERR_BAD_ARGUMENT;
    if (params_numel != score_layout(c1, c2).numel || ((uintptr_t)params & 15)) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!reg_fc_out || !yaw || !t_vec || !pose_cov || !dimensions || !params || !scores) return MR_ERR_BAD_ARGUMENT;
    ScoreArgs a;
    a.reg = reg_fc_out; a.yaw = yaw; a.t = t_vec; a.cov = pose_cov; a.dim = dimensions;
    a.reg_stride = reg_fc_out_row_stride; a.yaw_stride = yaw_row_stride; a.t_stride = t_vec_row_stride; a.dim_stride = dimensions_row_stride;
    a.ret_val = ret_val; a.scores_2d = scores_2d; a.params = params; a.n = n; a.c1 = c1; a.c2 = c2;
    a.sigmoid = (flags & MR_SCORE_SIGMOID) ? 1 : 0; a.out = scores;
    hipLaunchKernelGGL(score_head_forward_kernel, dim3((unsigned)(((long long)n + kScoreRows - 1) / kScoreRows)), dim3(kScoreThreads), 0,
                       (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
