/*
 * monorun_image.h — C ABI of the image preparation in libmonorun_pnp.so: what the reference's data pipeline runs on the CPU between the
 * loaded uint8 image and the collated batch — RandomFlip3D of the image and of the coord_2d field, mmdet's PhotoMetricDistortion,
 * Normalize, Pad3D and collate's zero padding to the batch shape — for a batch of N images of unequal sizes in ONE launch (DESIGN.md
 * section 26).  The entry point is compiled into the same library as those of monorun_pnp.h and follows its conventions: 0 on success or a
 * negative MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernel, in stream order, unless
 * it is called a HOST array below (read before the call returns); a call runs on the current HIP device, asynchronously on `stream`;
 * nothing is allocated and nothing synchronises, so a call can be captured into a graph.
 */
#ifndef MONORUN_IMAGE_H_
#define MONORUN_IMAGE_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_IMAGE_THREADS 256                /* threads of a workgroup; a thread owns four consecutive output columns of one row */
#define MR_IMAGE_MAX_IMAGES 65535           /* n_images: the images are the grid's second dimension */
#define MR_IMAGE_MAX_PIXELS 2147483647      /* batch_h * batch_w: 32-bit indexing inside an image's planes */
#define MR_IMAGE_PREPARE_LDS_BYTES 0        /* nothing is staged in LDS */

/*
 * The per-image table: MR_IMAGE_TABLE_WORDS 32-bit words per image, the float parameters stored by their bit patterns.
 */
#define MR_IMAGE_TABLE_WORDS 16
#define MR_IMAGE_OFFSET_LO 0                /* the byte offset of pixel (0, 0) in `src`, a non-negative 64-bit integer: low word, */
#define MR_IMAGE_OFFSET_HI 1                /* high word */
#define MR_IMAGE_H 2
#define MR_IMAGE_W 3
#define MR_IMAGE_STRIDE 4                   /* bytes from one row to the next, >= 3 w */
#define MR_IMAGE_FLIP 5                     /* not 0: horizontal flip */
#define MR_IMAGE_SWITCHES 6                 /* the MR_IMAGE_SW_* bits */
#define MR_IMAGE_PERMUTATION 7              /* p0 | p1 << 2 | p2 << 4: output channel c is the chain's channel p_c; identity: 0x24 */
#define MR_IMAGE_BRIGHTNESS_DELTA 8         /* float bits */
#define MR_IMAGE_CONTRAST_ALPHA 9
#define MR_IMAGE_SATURATION_ALPHA 10
#define MR_IMAGE_HUE_DELTA 11               /* words 12 .. 15: reserved, 0 */
#define MR_IMAGE_PERMUTATION_IDENTITY 0x24

#define MR_IMAGE_SW_BRIGHTNESS 0x1          /* step 1 */
#define MR_IMAGE_SW_CONTRAST 0x2            /* step 2 or 7, by MR_IMAGE_SW_CONTRAST_FIRST */
#define MR_IMAGE_SW_CONTRAST_FIRST 0x4      /* mmdet's mode 1: the contrast factor before the HSV round trip; clear: mode 0, after it */
#define MR_IMAGE_SW_SATURATION 0x8          /* step 4; needs MR_IMAGE_SW_HSV */
#define MR_IMAGE_SW_HUE 0x10                /* step 5; needs MR_IMAGE_SW_HSV */
#define MR_IMAGE_SW_HSV 0x20                /* steps 3 and 6: the round trip, which mmdet runs whenever PhotoMetricDistortion runs */
#define MR_IMAGE_SW_ALL 0x3f

/*
 * mr_image_prepare.  src: ONE packed buffer of src_bytes bytes holding the N = n_images uint8 images, HWC with 3 channels in B, G, R order
 * (mmcv.imread's), image n's pixel (y, x) channel k at byte offset_n + y stride_n + 3 x + k.  table: a HOST array of N rows of
 * MR_IMAGE_TABLE_WORDS words, which the call validates; table_device: the same rows in device memory, which the kernel reads (the caller
 * fills it through pinned memory in stream order, no blocking copy).  mean, std: HOST arrays of 3 doubles, indexed by OUTPUT plane;
 * to_rgb: not 0 reverses the channel order before the normalisation.  size_divisor: Pad3D's, a positive multiple of 4.  (batch_h,
 * batch_w): the batch shape, multiples of size_divisor and at least every image's padded shape.
 *
 * Outputs img (N, 3, batch_h, batch_w) and coord_2d (N, 2, batch_h, batch_w), fp32, contiguous, 16-byte aligned.  Per output pixel
 * (n, y, x), with hp, wp = h_n, w_n rounded up to size_divisor:
 *   y < h, x < w:          the source pixel is (y, xs), xs = w - 1 - x when flipped, else x.  (b, g, r) = its bytes as fp32, through the
 *                          chain below; q_c = the chain's channel p_c; plane c of img = (q_k - (float)mean[c]) * (float)(1.0 / std[c])
 *                          with k = 2 - c when to_rgb, else c.  coord_2d = [xs, y].
 *   else y < hp, x < wp:   img = 0; coord_2d replicates the last row and column (Pad3D's padding_mode='edge'):
 *                          [xs(min(x, w - 1)), min(y, h - 1)]
 *   else:                  img = 0, coord_2d = 0 (collate's padding)
 * The chain (mmdet's PhotoMetricDistortion on a float32 BGR pixel, no clipping anywhere), each step under its switch:
 *   1  b, g, r += brightness_delta
 *   2  CONTRAST and CONTRAST_FIRST: b, g, r *= contrast_alpha
 *   3  HSV:  V = max(b, g, r), d = V - min(b, g, r), S = d / (|V| + FLT_EPSILON), k = (float)(60.0 / (double)(d + FLT_EPSILON)),
 *            H = (g - b) k if V == r, else (b - r) k + 120 if V == g, else (r - g) k + 240;  H += 360 if H < 0
 *   4  S *= saturation_alpha
 *   5  H += hue_delta;  H -= 360 if H > 360;  H += 360 if H < 0
 *   6  HSV:  S == 0: b = g = r = V.  Else hs = H * (float)(6.0 / 360.0), sector = floorf(hs), f = hs - sector, a sector outside 0 .. 5
 *            becomes sector 0 with f = 0; tab = [V, V (1 - S), V (1 - S f), V (1 - S (1 - f))]; (b, g, r) = tab[row[sector]] with the
 *            rows {1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}
 *   7  CONTRAST without CONTRAST_FIRST: b, g, r *= contrast_alpha
 * Every operation is an IEEE fp32 one (the one division of step 3 that is stated in double excepted), rounded on its own in the order
 * written, contraction off: the result is bitwise a function of the inputs.  The conversions are OpenCV's float32 formulas as this
 * project states them; they are its definition and are not pinned against OpenCV.
 *
 * ONE launch; every element of both outputs is stored exactly once, by 16-byte stores: no memset, no atomics.  Every source byte read lies
 * at offset + y stride + 3 x + k with 0 <= y < h, 0 <= x < w, 0 <= k < 3.  n_images = 0 launches nothing and returns 0.
 *
 * MR_ERR_BAD_ARGUMENT, without a launch, for: n_images < 0; a size_divisor that is not a positive multiple of 4; batch_h or batch_w not a
 * positive multiple of size_divisor; a NULL mean or std, a std that is not a positive finite number, a mean that is not finite; and with
 * n_images > 0 a NULL pointer, an output not 16-byte aligned, src_bytes < 0, or a table row with h or w < 1, stride < 3 w, a negative
 * offset, offset + (h - 1) stride + 3 w > src_bytes, hp > batch_h or wp > batch_w, switch bits outside MR_IMAGE_SW_ALL, SATURATION or HUE
 * without HSV, a permutation word that is not one of the six, or a parameter that is not finite.  MR_ERR_UNSUPPORTED for n_images >
 * MR_IMAGE_MAX_IMAGES or batch_h batch_w > MR_IMAGE_MAX_PIXELS.
 */
int mr_image_prepare(const uint8_t *src, int64_t src_bytes, const int32_t *table, const int32_t *table_device, int n_images,
                     const double *mean, const double *std, int to_rgb, int size_divisor, int batch_h, int batch_w, float *img,
                     float *coord_2d, void *stream);

#ifdef __cplusplus
}
#endif
#endif
