/*
 * monorun_roi.h — C ABI of the multi-level RoI feature extractor in libmonorun_pnp.so: mmdet's SingleRoIExtractor over mmcv's RoIAlign
 * (average pooling), all levels and RoIs in ONE launch each way.  The entry points are compiled into the same
 * library as those of monorun_pnp.h and follow its conventions: 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data
 * pointer is a DEVICE pointer, dereferenced only by the kernel, in stream order; a call runs on the current HIP device, asynchronously
 * on `stream`; nothing is allocated.  The per-level arrays (feats / grad_feats, level_h, level_w, level_stride) are HOST arrays of
 * n_levels entries, read before the call returns: the level table travels in the kernel arguments.
 *
 * Reference interface replaced: mmdet.models.roi_heads.roi_extractors.SingleRoIExtractor with roi_layer RoIAlign (mmcv.ops.roi_align, a
 * CUDA extension with no ROCm build), which MonoRUnRoIHead builds as its bbox_roi_extractor and noc_roi_extractor.
 */
#ifndef MONORUN_ROI_H_
#define MONORUN_ROI_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ROI_MAX_LEVELS 8         /* n_levels */
#define MR_ROI_MAX_OUT 32           /* out_h, out_w */
#define MR_ROI_CHUNK 32             /* channels of one forward workgroup */
#define MR_ROI_TAPS 256             /* per-axis (bin, sample) records of the forward's LDS geometry table */
#define MR_ROI_TILE_H 8             /* the backward's map tile: one pixel per thread */
#define MR_ROI_TILE_W 32
#define MR_ROI_BWD_CHUNK 8          /* channels of one backward workgroup */
#define MR_ROI_FORWARD_LDS_BYTES (2 * MR_ROI_TAPS * 16)
#define MR_ROI_BACKWARD_LDS_BYTES (4 * ((MR_ROI_TILE_H + MR_ROI_TILE_W) * MR_ROI_MAX_OUT + MR_ROI_MAX_OUT * MR_ROI_MAX_OUT * MR_ROI_BWD_CHUNK + 256 + 4))

/*
 * The op.  feats[l] (n_images, channels, level_h[l], level_w[l]) fp32 contiguous, l < n_levels; rois (n_rois, 5) fp32 contiguous =
 * [image, x1, y1, x2, y2]; out (n_rois, channels, out_h, out_w) fp32 contiguous.  Per RoI, every operation an IEEE fp32 one:
 *   v      = sqrtf((x2 - x1) (y2 - y1)) / finest_scale + 1e-6f      of level_rois[k] (the same layout; NULL: of rois[k] — mmdet's
 *            roi_scale_factor rescales the RoIs AFTER the level rule: rois are then the rescaled boxes, level_rois the original ones)
 *   level  = the number of i in 1 .. n_levels - 1 with v >= 2^i                (a NaN v: level 0; n_levels 1: level 0)
 *   out[k] = mr_roi_align_avg's pooling of feats[level][(int)image] with spatial_scale 1 / level_stride[level], sampling_ratio and aligned
 * bit for bit (the same device routines; per element the samples are added iy outer, ix inner and divided by their count once).  A
 * DEGENERATE RoI gives zeros: a coordinate or image that is not finite, an image <= -1 or >= n_images, or at sampling_ratio 0 a sample grid
 * ceilf(roi_h / out_h) > level_h + 2 or ceilf(roi_w / out_w) > level_w + 2 (compared in float): the one deviation from mmcv, whose loops
 * such a RoI would leave unbounded.  ONE launch, no host synchronisation.
 *
 * n_rois = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for n_levels, n_images, channels, out_h, out_w, a level size or stride
 * < 1, n_rois or sampling_ratio < 0, a finest_scale that is not positive, or a NULL pointer; MR_ERR_UNSUPPORTED for n_levels >
 * MR_ROI_MAX_LEVELS, out_h or out_w > MR_ROI_MAX_OUT, an (image, level) slab channels level_h level_w or an output n_rois channels out_h
 * out_w of more than 2^31 - 1 elements, or more than 2^31 - 1 workgroups.
 */
int mr_roi_extract_forward(const float *const *feats, const int *level_h, const int *level_w, const int *level_stride, int n_levels,
                           int n_images, int channels, const float *rois, const float *level_rois, int n_rois, float finest_scale,
                           int out_h, int out_w, int sampling_ratio, int aligned, float *out, void *stream);

/*
 * mr_roi_extract_backward: the gradient of mr_roi_extract_forward's out to every feats[l] (rois get none), from rois and grad_out (out's
 * shape) alone.  ONE launch, a gather: every element of every grad_feats[l] (feats[l]'s shape) is stored exactly once — exact zeros where no
 * RoI reaches, whole levels and images included —, so the buffers need no memset; no atomics: each map pixel adds its RoIs in index order,
 * per RoI  (sum over ph, pw of (Wy[row][ph] Wx[col][pw]) grad_out[k, c, ph, pw]) / count  with the separable bilinear weights summed
 * over the bin's samples, bitwise reproducible.  n_rois = 0 stores zeros.  Errors as mr_roi_extract_forward.
 */
int mr_roi_extract_backward(const float *grad_out, const float *rois, const float *level_rois, int n_rois, float *const *grad_feats,
                            const int *level_h, const int *level_w, const int *level_stride, int n_levels, int n_images, int channels,
                            float finest_scale, int out_h, int out_w, int sampling_ratio, int aligned, void *stream);

#ifdef __cplusplus
}
#endif
#endif
