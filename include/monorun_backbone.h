/*
 * monorun_backbone.h — C ABI of the backbone's fused frozen-statistics batch norm in libmonorun_pnp.so: what a ResNet whose norms use
 * their running statistics (mmdet's `norm_eval=True`, every reference config) runs after each convolution — the per-channel affine map,
 * the residual add and the ReLU in ONE launch, their backward in one or two, and the stem's norm, ReLU and 3x3 / stride-2 max pooling in
 * one.  The entry points are compiled into the same library as those of monorun_pnp.h and follow the conventions
 * of monorun_fpn.h: 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only
 * by the kernels, in stream order; a call runs on the current HIP device, asynchronously on `stream`; nothing is allocated, nothing is
 * memset, no atomics are used and the host is never synchronised.  Every data pointer may have ANY 4-byte alignment.
 */
#ifndef MONORUN_BACKBONE_H_
#define MONORUN_BACKBONE_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_BN_THREADS 256           /* lanes of a streaming workgroup */
#define MR_BN_CHUNK 4096            /* elements of one (image, channel) plane that a streaming workgroup handles at a time */
#define MR_BN_MAX_GRID 2048         /* workgroups of a streaming launch at the most: each strides over the chunks */
#define MR_BN_FINAL_THREADS 64      /* lanes of a finalise workgroup: one wave per channel */
#define MR_BN_FORWARD_LDS_BYTES 0
#define MR_BN_WAVES 4               /* MR_BN_THREADS / 64 */
#define MR_BN_BACKWARD_LDS_BYTES (4 * 2 * MR_BN_WAVES)      /* one pair per wave, with the parameter gradients */
#define MR_BN_FINAL_LDS_BYTES 0
#define MR_STEM_TILE_H 8            /* the stem kernel's tile of the POOLED map: one (image, channel) plane per workgroup and tile */
#define MR_STEM_TILE_W 64
#define MR_STEM_THREADS 256
#define MR_STEM_LDS_BYTES (4 * (2 * MR_STEM_TILE_H + 1) * (2 * MR_STEM_TILE_W + 1))

/*
 * The op.  x (n_images, channels, height, width) fp32 contiguous; mean, var (channels), weight and bias (channels, or NULL); r of x's
 * shape or NULL.  Every operation is an IEEE fp32 one rounded on its own (contraction off); the square root and the division are the
 * correctly rounded ones.  With c the channel of an element:
 *   istd[c] = 1.0f / sqrtf(var[c] + (float)eps)
 *   xhat = (x - mean[c]) * istd[c]
 *   t = xhat * weight[c] + bias[c]              a NULL weight skips the multiplication, a NULL bias the addition
 *   u = t + r                                   without r: u = t
 *   y = relu ? (u <= 0 ? +0.0f : u) : u         NaN propagates; under relu a zero of either sign becomes +0.0f
 *
 * mr_bn_act_forward writes y (x's shape; y may be x or r itself: every element is read before it is written, by the same lane).  ONE
 * launch: a stream.  A plane (one image, one channel: height * width contiguous elements) is cut into chunks of MR_BN_CHUNK elements
 * counted from the plane's start, the last one shorter; a workgroup takes a chunk at a time (the channel is uniform over it: no
 * per-element division), min(chunks, MR_BN_MAX_GRID) workgroups stride over the chunks.  Within a chunk the elements up to the first
 * whose index IN THE TENSOR is a multiple of 4 (at most 3: the head) and those after the last such group of 4 (the tail) are accessed
 * 4 bytes at a time, the groups between them 16 bytes per lane through every pointer that is 16-byte aligned, and as four 4-byte accesses
 * through one that is not.
 *
 * MR_ERR_BAD_ARGUMENT: a size < 1, NULL x, mean, var or y, a relu flag other than 0 and 1, an eps that is negative or not finite.
 * MR_ERR_UNSUPPORTED: 2^31 elements or more.
 */
int mr_bn_act_forward(const float *x, const float *mean, const float *var, const float *weight, const float *bias, const float *r,
                      int n_images, int channels, int height, int width, double eps, int relu, float *y, void *stream);

/*
 * The backward, from g = d/dy, the saved y (read only under relu; may be NULL without) and the saved x (read only when a parameter
 * gradient is asked for; may be NULL otherwise):
 *   gm = relu ? (y <= 0 ? +0.0f : g) : g
 *   grad_r = gm
 *   grad_x = gm * k[c],   k[c] = istd[c] * weight[c] rounded once (NULL weight: k[c] = istd[c])
 *   grad_bias[c] = SUM gm,   grad_weight[c] = SUM gm * xhat    over the images and the plane, xhat = (x - mean[c]) * istd[c] as above,
 *                                                                 the product rounded before it is added
 * grad_x, grad_r, grad_weight and grad_bias may each be NULL: such an output is neither computed for storage nor stored.  With all four
 * NULL nothing is launched.  Without grad_weight and grad_bias: ONE launch, the stream of the forward.  With either: TWO launches and a
 * workspace of mr_bn_act_backward_workspace_bytes (4-byte aligned, contents undefined before and after).
 *
 * THE ORDER OF THE TWO SUMS depends on the shape alone.  Both sums add the same way; `term` is gm, or the rounded gm * xhat.
 *   1. A partial per chunk (above), (image, channel, chunk k of the plane).  Let f0 be the index in the tensor of the chunk's first
 *      element and n its length; head = min((4 - f0 % 4) % 4, n), groups = (n - head) / 4, the tail is the rest (at most 3).  Lane t of
 *      MR_BN_THREADS starts its accumulator at +0.0f and adds, in this order: head element t (if t < head); for v = t, t + 256, ... <
 *      groups, the four elements of group v in ascending order; tail element t (if there is one).
 *   2. The 256 accumulators: within each wave of 64 lanes a butterfly, a[i] = a[i] + a[i ^ d] for d = 32, 16, 8, 4, 2, 1; then the four
 *      waves' totals in ascending order from +0.0f.  The streaming launch stores this pair per chunk into the workspace.
 *   3. Per channel (the second launch: one wave of MR_BN_FINAL_THREADS lanes per channel): its partials in the order q = image *
 *      chunks_per_plane + k, P = n_images * chunks_per_plane of them.  Lane t starts at +0.0f and adds the partials q = t, t + 64, ...;
 *      then the butterfly of step 2 over the 64 lanes.
 * The longest chain of additions is therefore
 *   D = (2 + 4 * MR_BN_CHUNK / (4 * MR_BN_THREADS)) + 6 + 4 + ceil(P / 64) + 6 = 34 + ceil(P / 64)        (MR_BN_CHUNK = 4096)
 * and either sum differs from the exact sum of its fp32 terms by at most (D + 1) 2^-24 SUM |term|.
 *
 * Errors as mr_bn_act_forward; MR_ERR_BAD_ARGUMENT also for NULL g, NULL y under relu, NULL x or workspace with a parameter gradient.
 */
size_t mr_bn_act_backward_workspace_bytes(int n_images, int channels, int height, int width);
int mr_bn_act_backward(const float *g, const float *y, const float *x, const float *mean, const float *var, const float *weight,
                       int n_images, int channels, int height, int width, double eps, int relu, float *grad_x, float *grad_r,
                       float *grad_weight, float *grad_bias, void *workspace, void *stream);

/*
 * The stem: p (n_images, channels, out_h, out_w) = max_pool2d(y, kernel 3, stride 2, padding 1) of the y above with relu = 1 and no
 * r; out_h = (height - 1) / 2 + 1, out_w alike.  The full-resolution y is never written.
 *   p[oy, ox]: m = -inf; for dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner): iy = 2 oy + dy, ix = 2 ox + dx; a tap outside the map is
 *   skipped (padding takes no part); v = y[iy, ix]; m = (v > m || v != v) ? v : m.  NaN propagates; the centre tap is always inside.
 * ONE launch: a workgroup stages the (2 MR_STEM_TILE_H + 1) x (2 MR_STEM_TILE_W + 1) window of y under an MR_STEM_TILE_H x MR_STEM_TILE_W
 * tile of p in LDS, so that every element of x is fetched once per workgroup, and pools from LDS; min(tiles, MR_BN_MAX_GRID) workgroups
 * stride over the tiles.  Forward only.  Errors as mr_bn_act_forward (weight and bias may be NULL; p must not be).
 */
int mr_bn_relu_maxpool_forward(const float *x, const float *mean, const float *var, const float *weight, const float *bias,
                               int n_images, int channels, int height, int width, double eps, float *p, void *stream);

#ifdef __cplusplus
}
#endif
#endif
