// include/monorun_image.h: the image preparation, from the packed uint8 images to the normalised, padded batch and its coord_2d
static bool image_finite(float v) { return v - v == 0.0f; }

int mr_image_prepare(const uint8_t *src, int64_t src_bytes, const int32_t *table, const int32_t *table_device, int n_images,
                     const double *mean, const double *std, int to_rgb, int size_divisor, int batch_h, int batch_w, float *img,
                     float *coord_2d, void *stream) {
    static_assert(kImageThreads == MR_IMAGE_THREADS && kImageWords == MR_IMAGE_TABLE_WORDS && MR_IMAGE_PREPARE_LDS_BYTES == 0,
                  "the header states the launch");
    if (n_images < 0 || size_divisor < 4 || size_divisor % 4 != 0) return MR_ERR_BAD_ARGUMENT;
    if (batch_h < size_divisor || batch_w < size_divisor || batch_h % size_divisor != 0 || batch_w % size_divisor != 0) return MR_ERR_BAD_ARGUMENT;
    if (!mean || !std) return MR_ERR_BAD_ARGUMENT;
    for (int c = 0; c < 3; ++c)
        if (!(std[c] > 0.0) || !(std[c] - std[c] == 0.0) || !(mean[c] - mean[c] == 0.0)) return MR_ERR_BAD_ARGUMENT;
    if (n_images > MR_IMAGE_MAX_IMAGES || (long long)batch_h * batch_w > (long long)MR_IMAGE_MAX_PIXELS) return MR_ERR_UNSUPPORTED;
    if (n_images == 0) return MR_OK;
    if (!src || !table || !table_device || !img || !coord_2d || src_bytes < 0) return MR_ERR_BAD_ARGUMENT;
    if ((uintptr_t)img % 16 != 0 || (uintptr_t)coord_2d % 16 != 0) return MR_ERR_BAD_ARGUMENT;
    for (int n = 0; n < n_images; ++n) {
        const int32_t *t = table + (size_t)n * kImageWords;
        const long long off = (long long)(uint32_t)t[MR_IMAGE_OFFSET_LO] | ((long long)t[MR_IMAGE_OFFSET_HI] << 32);
        const long long h = t[MR_IMAGE_H], w = t[MR_IMAGE_W], stride = t[MR_IMAGE_STRIDE];
        if (h < 1 || w < 1 || stride < 3 * w || off < 0) return MR_ERR_BAD_ARGUMENT;
        if (off > (long long)src_bytes || (h - 1) * stride + 3 * w > (long long)src_bytes - off) return MR_ERR_BAD_ARGUMENT;
        if ((h + size_divisor - 1) / size_divisor * size_divisor > batch_h || (w + size_divisor - 1) / size_divisor * size_divisor > batch_w)
            return MR_ERR_BAD_ARGUMENT;
        const int sw = t[MR_IMAGE_SWITCHES], p = t[MR_IMAGE_PERMUTATION];
        if (sw & ~MR_IMAGE_SW_ALL) return MR_ERR_BAD_ARGUMENT;
        if ((sw & (MR_IMAGE_SW_SATURATION | MR_IMAGE_SW_HUE)) && !(sw & MR_IMAGE_SW_HSV)) return MR_ERR_BAD_ARGUMENT;
        const int p0 = p & 3, p1 = (p >> 2) & 3, p2 = (p >> 4) & 3;
        if ((p & ~0x3f) || ((1 << p0) | (1 << p1) | (1 << p2)) != 7) return MR_ERR_BAD_ARGUMENT;
        for (int k = MR_IMAGE_BRIGHTNESS_DELTA; k <= MR_IMAGE_HUE_DELTA; ++k) {
            float v;
            memcpy(&v, t + k, sizeof v);
            if (!image_finite(v)) return MR_ERR_BAD_ARGUMENT;
        }
    }
    ImagePrepArgs a;
    memset(&a, 0, sizeof a);
    a.src = src; a.table = (const int *)table_device;
    for (int c = 0; c < 3; ++c) { a.mean[c] = (float)mean[c]; a.inv_std[c] = (float)(1.0 / std[c]); }
    a.to_rgb = to_rgb ? 1 : 0; a.divisor = size_divisor; a.Hb = batch_h; a.Wb = batch_w;
    a.img = img; a.coord = coord_2d;
    const long long quads = (long long)batch_h * (batch_w / 4);
    const dim3 grid((unsigned)((quads + kImageThreads - 1) / kImageThreads), (unsigned)n_images);
    hipLaunchKernelGGL(image_prepare_kernel, grid, dim3(kImageThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
