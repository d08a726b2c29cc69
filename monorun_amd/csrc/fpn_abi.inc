// include/monorun_fpn.h: the feature pyramid's top-down pathway (mmdet's FPN, the reference's FPNplus)
static int fpn_fill(FpnArgs &a, const int *level_h, const int *level_w, int n_levels, int n_images, int channels, int lower_scale) {
    static_assert(kFpnMaxLevels == MR_FPN_MAX_LEVELS && kFpnTileH == MR_FPN_TILE_H && kFpnTileW == MR_FPN_TILE_W && kFpnFlat == MR_FPN_FLAT &&
                  kFpnBwdEven == MR_FPN_BWD_EVEN && kFpnBwdOdd == MR_FPN_BWD_ODD && kFpnBwdRows == MR_FPN_BWD_ROWS && kFpnBwdCols == MR_FPN_BWD_COLS, "the header states the tiling");
    static_assert(sizeof(float) * (kFpnTileH + 2) * (kFpnTileW + 2) == MR_FPN_FORWARD_LDS_BYTES &&
                  sizeof(FpnBwdLds) == MR_FPN_BACKWARD_LDS_BYTES, "the header states the LDS");
    if (n_levels < 1 || n_images < 1 || channels < 1 || (lower_scale != 0 && lower_scale != 2) || !level_h || !level_w) return MR_ERR_BAD_ARGUMENT;
    for (int l = 0; l < n_levels; ++l)
        if (level_h[l] < 1 || level_w[l] < 1) return MR_ERR_BAD_ARGUMENT;
    if (n_levels > kFpnMaxLevels || (long long)n_images * channels > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    memset(&a, 0, sizeof a);
    for (int l = 0; l < n_levels; ++l) {
        const long long slab = (long long)channels * level_h[l] * level_w[l];
        if (slab > 0x7fffffffLL || (l == 0 && lower_scale && 4 * slab > 0x7fffffffLL)) return MR_ERR_UNSUPPORTED;
        a.lv[l].H = level_h[l]; a.lv[l].W = level_w[l]; a.lv[l].ry = a.lv[l].rx = 1.0f;
        if (l + 1 < n_levels) {         // the pyramid rule
            const long long h = level_h[l], w = level_w[l], hp = level_h[l + 1], wp = level_w[l + 1];
            if (hp > h || h > 2 * hp || wp > w || w > 2 * wp) return MR_ERR_UNSUPPORTED;
            a.lv[l].ry = (float)level_h[l + 1] / (float)level_h[l];
            a.lv[l].rx = (float)level_w[l + 1] / (float)level_w[l];
        }
    }
    a.L = n_levels; a.planes = n_images * channels; a.lower = lower_scale ? 1 : 0;
    return MR_OK;
}

int mr_fpn_topdown_forward(const float *const *lat, const int *level_h, const int *level_w, int n_levels, int n_images, int channels,
                           int lower_scale, float *const *merged, float *low, void *stream) {
    FpnArgs a;
    const int rc = fpn_fill(a, level_h, level_w, n_levels, n_images, channels, lower_scale);
    if (rc != MR_OK) return rc;
    if (!lat || (n_levels > 1 && !merged) || (lower_scale && !low)) return MR_ERR_BAD_ARGUMENT;
    long long blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (!lat[l] || (l + 1 < n_levels && !merged[l])) return MR_ERR_BAD_ARGUMENT;
        a.lv[l].in = lat[l]; a.lv[l].out = l + 1 < n_levels ? merged[l] : nullptr;
        if (blocks > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
        a.lv[l].first_block = (unsigned)blocks;
        const long long hw = (long long)a.lv[l].H * a.lv[l].W;
        if (l == 0 && a.lower)
            blocks += (long long)a.planes * ((a.lv[0].H + kFpnTileH - 1) / kFpnTileH) * ((a.lv[0].W + kFpnTileW - 1) / kFpnTileW);
        else if (l + 1 < n_levels)
            blocks += (a.planes * hw + kFpnFlat - 1) / kFpnFlat;
    }
    if (blocks > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    if (blocks == 0) return MR_OK;          // one level and no lower map: m[0] is lat[0]
    a.low = low;
    a.low_vec = a.lv[0].W % 2 == 0 && (uintptr_t)low % 16 == 0 ? 4 : (uintptr_t)low % 8 == 0 ? 2 : 1;
    hipLaunchKernelGGL(fpn_topdown_forward_kernel, dim3((unsigned)blocks), dim3(kFpnThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_fpn_topdown_backward(const float *const *grad_merged, const float *grad_low, const int *level_h, const int *level_w, int n_levels,
                            int n_images, int channels, int lower_scale, float *const *grad_lat, void *stream) {
    FpnArgs a;
    const int rc = fpn_fill(a, level_h, level_w, n_levels, n_images, channels, lower_scale);
    if (rc != MR_OK) return rc;
    if (!grad_lat) return MR_ERR_BAD_ARGUMENT;
    for (int l = 0; l < n_levels; ++l) { a.lv[l].in = grad_merged ? grad_merged[l] : nullptr; a.lv[l].out = grad_lat[l]; }
    a.grad_low = grad_low;
    // the block of coarsest pixels of a workgroup: what a 16 x 64 footprint on level 0 comes from when every level halves
    a.root_h = kFpnTileH >> (n_levels - 1) > 1 ? kFpnTileH >> (n_levels - 1) : 1;
    a.root_w = kFpnTileW >> (n_levels - 1) > 1 ? kFpnTileW >> (n_levels - 1) : 1;
    // every footprint fits its LDS buffer: the largest extent per axis and level over the blocks, by the kernel's own routine.  Under the
    // pyramid rule k parents have at most 2k + 1 children, which the buffers are sized for; the check keeps the kernel inside them
    // whatever the rounding of the rule does.
    const FpnLevel &root = a.lv[n_levels - 1];
    const int tiles_y = (root.H + a.root_h - 1) / a.root_h, tiles_x = (root.W + a.root_w - 1) / a.root_w;
    int max_h[kFpnMaxLevels] = {0}, max_w[kFpnMaxLevels] = {0};
    for (int axis = 0; axis < 2; ++axis)
        for (int t = 0; t < (axis ? tiles_x : tiles_y); ++t) {
            const int step = axis ? a.root_w : a.root_h, size = axis ? root.W : root.H;
            int lo = t * step, hi = lo + step < size ? lo + step : size;
            for (int l = n_levels - 1; l >= 0; --l) {
                if (l < n_levels - 1) {
                    const float r = axis ? a.lv[l].rx : a.lv[l].ry;
                    const int nc = axis ? a.lv[l].W : a.lv[l].H, np = axis ? a.lv[l + 1].W : a.lv[l + 1].H;
                    lo = fpn_first_child(lo, r, nc, np); hi = fpn_first_child(hi, r, nc, np);
                }
                int &m = axis ? max_w[l] : max_h[l];
                if (hi - lo > m) m = hi - lo;
            }
        }
    for (int l = 0; l < n_levels; ++l)
        if ((long long)max_h[l] * max_w[l] > ((l & 1) ? kFpnBwdOdd : kFpnBwdEven) || (l > 0 && (max_h[l] > kFpnBwdRows || max_w[l] > kFpnBwdCols)))
            return MR_ERR_UNSUPPORTED;
    const long long blocks = (long long)a.planes * tiles_y * tiles_x;
    if (blocks > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(fpn_topdown_backward_kernel, dim3((unsigned)blocks), dim3(kFpnThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
