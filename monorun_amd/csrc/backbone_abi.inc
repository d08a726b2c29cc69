// include/monorun_backbone.h: the backbone's fused frozen-statistics batch norm (mmdet's ResNet with norm_eval=True)
static int bn_fill(BnArgs &a, const float *mean, const float *var, int n_images, int channels, int height, int width, double eps, int relu) {
    static_assert(kBnThreads == MR_BN_THREADS && kBnWaves == MR_BN_WAVES && kBnChunk == MR_BN_CHUNK && kBnMaxGrid == MR_BN_MAX_GRID &&
                  kBnFinalThreads == MR_BN_FINAL_THREADS && kStemTileH == MR_STEM_TILE_H && kStemTileW == MR_STEM_TILE_W &&
                  kStemThreads == MR_STEM_THREADS, "the header states the tiling");
    static_assert(sizeof(float) * 2 * kBnWaves == MR_BN_BACKWARD_LDS_BYTES && sizeof(float) * kStemRows * kStemCols == MR_STEM_LDS_BYTES,
                  "the header states the LDS");
    if (n_images < 1 || channels < 1 || height < 1 || width < 1 || !mean || !var || (relu != 0 && relu != 1) || !(eps >= 0.0) || eps > 3.0e38)
        return MR_ERR_BAD_ARGUMENT;
    const long long total = (long long)n_images * channels * height * width;
    if ((long long)n_images * channels > 0x7fffffffLL || (long long)height * width > 0x7fffffffLL || total > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    memset(&a, 0, sizeof a);
    a.mean = mean; a.var = var; a.N = n_images; a.C = channels; a.HW = height * width; a.eps = (float)eps;
    a.chunks_per_plane = (a.HW + kBnChunk - 1) / kBnChunk;
    a.chunks = n_images * channels * a.chunks_per_plane;        // at most one per element
    return MR_OK;
}

static unsigned bn_vec(const void *p, unsigned bit) { return p && (uintptr_t)p % 16 == 0 ? bit : 0u; }

int mr_bn_act_forward(const float *x, const float *mean, const float *var, const float *weight, const float *bias, const float *r,
                      int n_images, int channels, int height, int width, double eps, int relu, float *y, void *stream) {
    BnArgs a;
    const int rc = bn_fill(a, mean, var, n_images, channels, height, width, eps, relu);
    if (rc != MR_OK) return rc;
    if (!x || !y) return MR_ERR_BAD_ARGUMENT;
    a.x = x; a.r = r; a.weight = weight; a.bias = bias; a.y = y;
    a.vec = bn_vec(x, kBnVecX) | bn_vec(r, kBnVecR) | bn_vec(y, kBnVecY);
    const dim3 grid((unsigned)(a.chunks < kBnMaxGrid ? a.chunks : kBnMaxGrid)), block(kBnThreads);
    hipStream_t st = (hipStream_t)stream;
    if (r) {
        if (relu) hipLaunchKernelGGL((bn_act_forward_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((bn_act_forward_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (relu) hipLaunchKernelGGL((bn_act_forward_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((bn_act_forward_kernel<false, false>), grid, block, 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

size_t mr_bn_act_backward_workspace_bytes(int n_images, int channels, int height, int width) {
    BnArgs a;
    const float one = 1.0f;
    if (bn_fill(a, &one, &one, n_images, channels, height, width, 0.0, 0) != MR_OK) return 0;
    return sizeof(float) * 2 * (size_t)a.chunks;
}

int mr_bn_act_backward(const float *g, const float *y, const float *x, const float *mean, const float *var, const float *weight,
                       int n_images, int channels, int height, int width, double eps, int relu, float *grad_x, float *grad_r,
                       float *grad_weight, float *grad_bias, void *workspace, void *stream) {
    BnArgs a;
    const int rc = bn_fill(a, mean, var, n_images, channels, height, width, eps, relu);
    if (rc != MR_OK) return rc;
    const bool params = grad_weight || grad_bias;
    if (!g || (relu && !y) || (params && (!x || !workspace))) return MR_ERR_BAD_ARGUMENT;
    if (!params && !grad_x && !grad_r) return MR_OK;
    a.g = g; a.y_in = relu ? y : nullptr; a.x = params ? x : nullptr; a.weight = weight; a.gx = grad_x; a.gr = grad_r;
    a.part = params ? (float *)workspace : nullptr; a.gw = grad_weight; a.gb = grad_bias;
    a.vec = bn_vec(g, kBnVecG) | bn_vec(a.y_in, kBnVecYin) | bn_vec(a.x, kBnVecX) | bn_vec(grad_x, kBnVecGx) | bn_vec(grad_r, kBnVecGr);
    const dim3 grid((unsigned)(a.chunks < kBnMaxGrid ? a.chunks : kBnMaxGrid)), block(kBnThreads);
    hipStream_t st = (hipStream_t)stream;
    if (params) {
        if (relu) hipLaunchKernelGGL((bn_act_backward_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((bn_act_backward_kernel<false, true>), grid, block, 0, st, a);
    } else {
        if (relu) hipLaunchKernelGGL((bn_act_backward_kernel<true, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((bn_act_backward_kernel<false, false>), grid, block, 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    if (params) {
        hipLaunchKernelGGL(bn_act_backward_final_kernel, dim3((unsigned)channels), dim3(kBnFinalThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return MR_OK;
}

int mr_bn_relu_maxpool_forward(const float *x, const float *mean, const float *var, const float *weight, const float *bias,
                               int n_images, int channels, int height, int width, double eps, float *p, void *stream) {
    BnArgs a;
    const int rc = bn_fill(a, mean, var, n_images, channels, height, width, eps, 1);
    if (rc != MR_OK) return rc;
    if (!x || !p) return MR_ERR_BAD_ARGUMENT;
    StemArgs s;
    memset(&s, 0, sizeof s);
    s.x = x; s.mean = mean; s.var = var; s.weight = weight; s.bias = bias; s.p = p; s.eps = (float)eps;
    s.C = channels; s.H = height; s.W = width; s.Ho = (height - 1) / 2 + 1; s.Wo = (width - 1) / 2 + 1;
    s.tiles_x = (s.Wo + kStemTileW - 1) / kStemTileW; s.tiles_y = (s.Ho + kStemTileH - 1) / kStemTileH;
    const long long tiles = (long long)n_images * channels * s.tiles_x * s.tiles_y;         // at most one per element
    s.tiles = (int)tiles;
    hipLaunchKernelGGL(bn_relu_maxpool_forward_kernel, dim3((unsigned)(tiles < kBnMaxGrid ? tiles : kBnMaxGrid)), dim3(kStemThreads), 0,
                       (hipStream_t)stream, s);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
