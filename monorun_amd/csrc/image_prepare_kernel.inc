// image_prepare_kernel.inc — the image preparation (DESIGN.md section 26; included by monorun_pnp.hip inside its anonymous namespace): the
// flip, mmdet's PhotoMetricDistortion, Normalize, Pad3D and collate's padding of a batch of unequal uint8 BGR images, with the coord_2d
// field, ONE launch.  A streaming pass: 3 bytes read per pixel, five fp32 planes written by 16-byte stores.  Contraction is off: every
// operation is an fp32 one in the order include/monorun_image.h states.  No LDS (MR_IMAGE_PREPARE_LDS_BYTES = 0).
constexpr int kImageThreads = 256;          // MR_IMAGE_THREADS
constexpr int kImageWords = 16;             // MR_IMAGE_TABLE_WORDS

struct ImagePrepArgs {
    const uint8_t *src;
    const int *table;                       // (N, kImageWords), device
    float mean[3], inv_std[3];              // by output plane
    int to_rgb, divisor, Hb, Wb;
    float *img, *coord;                     // (N, 3, Hb, Wb), (N, 2, Hb, Wb)
};

__device__ __forceinline__ float image_pick(float b, float g, float r, int i) { return i == 0 ? b : i == 1 ? g : r; }

// The chain of monorun_image.h on one pixel; `sw` and the four parameters are the same in every lane of a workgroup.
__device__ __forceinline__ void image_photometric(float &b, float &g, float &r, int sw, float brightness, float contrast, float saturation,
                                                  float hue) {
#pragma clang fp contract(off)
    if (sw & MR_IMAGE_SW_BRIGHTNESS) { b += brightness; g += brightness; r += brightness; }
    const bool contrast_on = sw & MR_IMAGE_SW_CONTRAST, first = sw & MR_IMAGE_SW_CONTRAST_FIRST;
    if (contrast_on && first) { b *= contrast; g *= contrast; r *= contrast; }
    if (sw & MR_IMAGE_SW_HSV) {
        const float V = fmaxf(b, fmaxf(g, r)), d = V - fminf(b, fminf(g, r));
        float S = d / (fabsf(V) + 1.1920929e-7f);
        const float k = (float)(60.0 / (double)(d + 1.1920929e-7f));
        float H = V == r ? (g - b) * k : V == g ? (b - r) * k + 120.0f : (r - g) * k + 240.0f;
        if (H < 0.0f) H += 360.0f;
        if (sw & MR_IMAGE_SW_SATURATION) S *= saturation;
        if (sw & MR_IMAGE_SW_HUE) {
            H += hue;
            if (H > 360.0f) H -= 360.0f;
            if (H < 0.0f) H += 360.0f;
        }
        if (S == 0.0f) {
            b = g = r = V;
        } else {
            const float hs = H * (float)(6.0 / 360.0);
            float fl = floorf(hs), f = hs - fl;
            if (!(fl >= 0.0f && fl <= 5.0f)) { fl = 0.0f; f = 0.0f; }
            const int s = (int)fl;
            const float t0 = V, t1 = V * (1.0f - S), t2 = V * (1.0f - S * f), t3 = V * (1.0f - S * (1.0f - f));
            // rows {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}: selects, no indexed array
            b = s <= 1 ? t1 : s == 2 ? t3 : s <= 4 ? t0 : t2;
            g = s == 0 ? t3 : s <= 2 ? t0 : s == 3 ? t2 : t1;
            r = s == 0 ? t0 : s == 1 ? t2 : s <= 3 ? t1 : s == 4 ? t3 : t0;
        }
    }
    if (contrast_on && !first) { b *= contrast; g *= contrast; r *= contrast; }
}

// Grid (ceil(Hb Wb / 4 / 256), N): blockIdx.y is the image, so its table row is read by scalar loads; a thread owns the four columns
// x0 .. x0 + 3 of one row.  Wb, wp and x0 are multiples of 4: a quad never straddles the padded shape, and its stores are 16-byte aligned.
// The source column is clamped to [0, w - 1] and the row is below h wherever a byte is read: every read stays inside the image's bytes.
__global__ void __launch_bounds__(kImageThreads) image_prepare_kernel(const ImagePrepArgs a) {
#pragma clang fp contract(off)
    const int n = blockIdx.y;
    const int *t = a.table + (size_t)n * kImageWords;
    const int Wq = a.Wb >> 2;
    const int q = blockIdx.x * kImageThreads + threadIdx.x;
    if (q >= a.Hb * Wq) return;
    const int y = q / Wq, x0 = (q - y * Wq) << 2;
    const int h = t[MR_IMAGE_H], w = t[MR_IMAGE_W], flip = t[MR_IMAGE_FLIP];
    const int hp = (h + a.divisor - 1) / a.divisor * a.divisor, wp = (w + a.divisor - 1) / a.divisor * a.divisor;
    float o[5][4];
#pragma unroll
    for (int c = 0; c < 5; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[c][j] = 0.0f;
    if (y < hp && x0 < wp) {
        const int yc = min(y, h - 1);
        int xs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xc = min(x0 + j, w - 1);
            xs[j] = flip ? w - 1 - xc : xc;
            o[3][j] = (float)xs[j];
            o[4][j] = (float)yc;
        }
        if (y < h && x0 < w) {
            const long long off = (long long)(unsigned)t[MR_IMAGE_OFFSET_LO] | ((long long)t[MR_IMAGE_OFFSET_HI] << 32);
            const uint8_t *row = a.src + off + (long long)y * t[MR_IMAGE_STRIDE];
            const int sw = t[MR_IMAGE_SWITCHES], perm = t[MR_IMAGE_PERMUTATION];
            const float brightness = __int_as_float(t[MR_IMAGE_BRIGHTNESS_DELTA]), contrast = __int_as_float(t[MR_IMAGE_CONTRAST_ALPHA]);
            const float saturation = __int_as_float(t[MR_IMAGE_SATURATION_ALPHA]), hue = __int_as_float(t[MR_IMAGE_HUE_DELTA]);
            int ch[3];                      // the chain's channel behind output plane c
#pragma unroll
            for (int c = 0; c < 3; ++c) ch[c] = (perm >> (2 * (a.to_rgb ? 2 - c : c))) & 3;
            uint8_t px[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 3; ++k) px[j][k] = row[3 * xs[j] + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float b = (float)px[j][0], g = (float)px[j][1], r = (float)px[j][2];
                if (sw) image_photometric(b, g, r, sw, brightness, contrast, saturation, hue);
                const bool in = x0 + j < w;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = (image_pick(b, g, r, ch[c]) - a.mean[c]) * a.inv_std[c];
                    o[c][j] = in ? v : 0.0f;
                }
            }
        }
    }
    const size_t plane = (size_t)a.Hb * a.Wb, at = (size_t)y * a.Wb + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4 *>(a.img + ((size_t)n * 3 + c) * plane + at) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
#pragma unroll
    for (int c = 0; c < 2; ++c)
        *reinterpret_cast<float4 *>(a.coord + ((size_t)n * 2 + c) * plane + at) = make_float4(o[3 + c][0], o[3 + c][1], o[3 + c][2], o[3 + c][3]);
}
