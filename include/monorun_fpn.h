/*
 * monorun_fpn.h — C ABI of the feature pyramid's top-down pathway in libmonorun_pnp.so: what mmdet's FPN and the reference's FPNplus
 * (monorun/models/necks/fpn_plus.py) run between their lateral 1x1 convolutions and their 3x3 output convolutions — per level a nearest
 * up-sample and an in-place add, and FPNplus' bilinear x2 up-sample of the merged finest level —, in ONE launch forward and ONE backward
 * (DESIGN.md section 22).  The entry points are compiled into the same library as those of monorun_pnp.h and follow the conventions of
 * monorun_roi.h: 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by
 * the kernel, in stream order; a call runs on the current HIP device, asynchronously on `stream`; nothing is allocated and the host is
 * never synchronised.  The per-level arrays (lat, merged, grad_merged, grad_lat, level_h, level_w) are HOST arrays of n_levels entries,
 * read before the call returns: the level table travels in the kernel arguments.
 */
#ifndef MONORUN_FPN_H_
#define MONORUN_FPN_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_FPN_MAX_LEVELS 6         /* n_levels */
#define MR_FPN_TILE_H 16            /* the forward's tile of the finest level when lower_scale = 2: one (image, channel) plane per workgroup */
#define MR_FPN_TILE_W 64
#define MR_FPN_FLAT 1024            /* elements of a forward workgroup on every other level */
#define MR_FPN_BWD_EVEN 6144        /* the backward's two LDS buffers, in floats: the footprints of the levels 0, 2, 4 and of 1, 3, 5 */
#define MR_FPN_BWD_ODD 1536
#define MR_FPN_BWD_ROWS 32           /* the largest footprint of a level that has children (l >= 1), per axis */
#define MR_FPN_BWD_COLS 48
#define MR_FPN_FORWARD_LDS_BYTES (4 * (MR_FPN_TILE_H + 2) * (MR_FPN_TILE_W + 2))
#define MR_FPN_BACKWARD_LDS_BYTES (4 * (MR_FPN_BWD_EVEN + MR_FPN_BWD_ODD + 4 * MR_FPN_MAX_LEVELS + MR_FPN_BWD_ROWS + 1 + MR_FPN_BWD_COLS + 1))

/*
 * The op.  lat[l] (n_images, channels, level_h[l], level_w[l]) fp32 contiguous, l < n_levels, FINEST FIRST; every operation an IEEE fp32
 * one, rounded on its own (contraction off).  With H = level_h[l], H' = level_h[l + 1] (W alike):
 *   m[L-1] = lat[L-1]
 *   m[l][y, x] = lat[l][y, x] + m[l+1][iy(y), ix(x)],   iy(y) = min((int)floorf(y * ((float)H' / (float)H)), H' - 1)      l = L-2 .. 0
 * (one add per level, coarsest first: bit for bit the in-place chain  lat[l] += F.interpolate(lat[l+1], size=lat[l].shape[2:],
 * mode='nearest')), and with lower_scale = 2, low (n_images, channels, 2 level_h[0], 2 level_w[0]) = the align_corners=False bilinear x2
 * up-sample of m[0]:
 *   src = max((Y + 0.5f) * 0.5f - 0.5f, 0),  i0 = (int)src,  i1 = i0 + (i0 < H - 1),  l1 = src - i0,  l0 = 1 - l1       (X alike)
 *   low[Y, X] = l0y * (l0x * m[i0y, i0x] + l1x * m[i0y, i1x]) + l1y * (l0x * m[i1y, i0x] + l1x * m[i1y, i1x])
 *
 * mr_fpn_topdown_forward writes merged[l] = m[l] for l < L - 1 (merged[L-1] is never read: m[L-1] IS lat[L-1], nothing is copied) and,
 * with lower_scale = 2, low.  ONE launch; with n_levels = 1 and lower_scale = 0 there is nothing to compute and nothing is launched.
 *
 * THE PYRAMID RULE.  level_h[l+1] <= level_h[l] <= 2 level_h[l+1] and the same for level_w, for every l: every level is between the
 * size of the finer one and half of it, rounded up.  Every pyramid of stride-2 convolutions with padding, level_h[l+1] =
 * ceil(level_h[l] / 2), satisfies it.  BOTH entry points enforce it, so that whatever the forward computed the backward can differentiate:
 * the backward's workgroups own the footprint of a block of coarsest pixels through all levels, and the rule bounds that footprint by
 * the LDS buffers above.
 *
 * MR_ERR_BAD_ARGUMENT for n_levels, n_images, channels or a level size < 1, a lower_scale other than 0 and 2, or a NULL pointer that is
 * needed (lat and each lat[l]; merged and merged[l] for l < L - 1; low with lower_scale = 2); MR_ERR_UNSUPPORTED for n_levels >
 * MR_FPN_MAX_LEVELS, a pyramid outside the rule, an (image, level) slab channels level_h level_w — or channels 4 level_h[0] level_w[0] of
 * low — of more than 2^31 - 1 elements, or more than 2^31 - 1 workgroups.
 */
int mr_fpn_topdown_forward(const float *const *lat, const int *level_h, const int *level_w, int n_levels, int n_images, int channels,
                           int lower_scale, float *const *merged, float *low, void *stream);

/*
 * mr_fpn_topdown_backward: the gradient to every lat[l] from the gradients grad_merged[l] arriving at m[l] (a NULL entry, or a NULL table,
 * counts as zeros) and grad_low arriving at low (NULL: zeros; ignored with lower_scale = 0).  With G[l] = grad_lat[l]:
 *   G[0][p] = grad_merged[0][p] + B,   B = the sum of (wy * wx) * grad_low[Y, X] over the at most 4 x 4 low pixels that read m[0][p] with a
 *             weight that is not zero, Y outer and X inner, ascending, into an accumulator that starts at 0; wy, wx: the sums of the
 *             forward's l0 / l1 with which row Y (column X) reads p.  (lower_scale = 0: G[0] = grad_merged[0], or zeros.)
 *   G[l][p] = grad_merged[l][p] + S,   S = the row-major running sum from 0 of G[l-1][q] over the children q of p: the pixels with
 *             (iy(q_y), ix(q_x)) = p, a contiguous rectangle that may be empty.
 * ONE launch, a gather: one workgroup owns the footprint of a block of coarsest pixels of one (image, channel) plane through all levels,
 * keeps each level's G in LDS for the next, and stores every element of every grad_lat[l] exactly once (a NULL grad_lat[l] is computed
 * and not stored): no atomics, no memset, bitwise reproducible.  Errors as mr_fpn_topdown_forward (grad_lat itself must not be NULL).
 */
int mr_fpn_topdown_backward(const float *const *grad_merged, const float *grad_low, const int *level_h, const int *level_w, int n_levels,
                            int n_images, int channels, int lower_scale, float *const *grad_lat, void *stream);

#ifdef __cplusplus
}
#endif
#endif
