// include/monorun_result3d.h: the per-image result tail, poses and scores to the class-grouped NMS result in one launch
int mr_result3d_nms(const float *dimensions, const float *yaw, const float *t_vec, const float *scores, const int64_t *labels,
                    const float *det_bboxes, int n, int num_classes, float thr, float *out3d, float *out2d, int64_t *keep_local,
                    int64_t *keep_row, int32_t *num_keep, int32_t *num_in_class, void *stream) {
    static_assert(kResult3dMaxN == MR_RESULT3D_MAX_N && kResult3dMaxN == kNmsMax && kResult3dMaxClasses == MR_RESULT3D_MAX_CLASSES &&
                  kResult3dThreads == MR_RESULT3D_THREADS && sizeof(NmsBox) == MR_RESULT3D_BOX_BYTES, "the header states the caps");
    static_assert(result3d_lds(kResult3dMaxN, 512) == MR_RESULT3D_MAX_LDS_BYTES && result3d_lds(33, 64) == MR_RESULT3D_LDS_BYTES(33, 64) &&
                  MR_RESULT3D_MAX_LDS_BYTES <= 64 * 1024, "the header states the LDS");
    if (n < 0 || num_classes < 0) return MR_ERR_BAD_ARGUMENT;
    if (n > kResult3dMaxN || num_classes > kResult3dMaxClasses) return MR_ERR_UNSUPPORTED;
    if (num_classes == 0) return MR_OK;
    if (!out3d || !out2d || !keep_local || !keep_row || !num_keep || !num_in_class) return MR_ERR_BAD_ARGUMENT;
    if (n > 0 && (!dimensions || !yaw || !t_vec || !scores || !labels || !det_bboxes)) return MR_ERR_BAD_ARGUMENT;
    if ((uintptr_t)out3d & 15) return MR_ERR_BAD_ARGUMENT;
    Result3dArgs a;
    a.dimensions = dimensions; a.yaw = yaw; a.t_vec = t_vec; a.scores = scores; a.det_bboxes = det_bboxes;
    a.labels = (const long long *)labels;
    a.N = n; a.C = num_classes; a.thr = thr;
    a.out3d = out3d; a.out2d = out2d; a.keep_local = (long long *)keep_local; a.keep_row = (long long *)keep_row;
    a.num_keep = (int *)num_keep; a.num_in_class = (int *)num_in_class;
    int np2 = 1; while (np2 < n) np2 <<= 1;
    hipLaunchKernelGGL(result3d_nms_kernel, dim3(num_classes), dim3(kResult3dThreads), result3d_lds(n, np2), (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
