/*
 * monorun_carafe.h — C ABI of the NOC head trunk's upsampler in libmonorun_pnp.so: CARAFEPack's kernel normaliser and feature reassembly,
 * fused.  The entry points are compiled into the same library as those of monorun_pnp.h and follow its conventions:
 * 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only by the kernel, in
 * stream order; a call runs on the current HIP device, asynchronously on `stream`; nothing is allocated.
 *
 * Reference interface replaced: mmcv.ops.carafe.CARAFEPack.kernel_normalizer + feature_reassemble (a CUDA extension with no ROCm build),
 * which FCNNOCDecoder of the MonoRUn tree builds as its `upsample` (monorun/models/roi_heads/bbox_3d_heads/dense_decoders/fcn_noc_decoder.py).
 */
#ifndef MONORUN_CARAFE_H_
#define MONORUN_CARAFE_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MR_CARAFE_MAX_KERNEL 7      /* up_kernel: odd, 1 .. 7 */
#define MR_CARAFE_TILE 16           /* source pixels per workgroup tile side */
#define MR_CARAFE_CHUNK 32          /* channels a workgroup stages in LDS at a time */

/*
 * The op.  x (n, channels, h, w) fp32 contiguous are the features, m (n, up_group k^2 s^2, h, w) fp32 contiguous the content encoder's raw
 * output (BEFORE the pixel shuffle), k = up_kernel, s = scale_factor, r = (k - 1) / 2, G = up_group, g = c / (channels / G).  Per output
 * pixel (ph, pw) of (h s, w s), with sub = (ph % s) s + pw % s and t = iy k + ix:
 *   l_t            = m[i, (g k^2 + t) s^2 + sub, ph / s, pw / s]                            (pixel_shuffle(m, s))
 *   w_t            = mr_expf(l_t - max_t l) / sum_t mr_expf(l_t - max_t l)                  (softmax over the k^2 taps of the group)
 *   out[i,c,ph,pw] = sum_t x[i, c, ph / s + iy - r, pw / s + ix - r] w_t                    (taps outside the map contribute zero)
 * in fp32; both sums run in one thread in the order of t (the second as a chain of fused multiply-adds), so a RoI's result does not depend
 * on the batch.  out (n, channels, h s, w s) fp32 contiguous; ONE launch, the shuffled logits and the masks never reach memory.
 *
 * n = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT for n < 0, channels, h, w or up_group < 1, a channels that up_group does not
 * divide or a NULL pointer; MR_ERR_UNSUPPORTED for an up_kernel that is not 1, 3, 5 or 7, a scale_factor that is not 1, 2 or 4, an output
 * map of more than 2^31 - 1 pixels or more than 2^31 - 1 workgroups.
 */
int mr_carafe_pack_forward(const float *x, const float *m, int n, int channels, int h, int w, int up_kernel, int up_group, int scale_factor,
                           float *out, void *stream);

/* Bytes of workspace mr_carafe_pack_backward needs to give grad_x: the normalised masks, 4 n up_group k^2 (h s) (w s); 0 for arguments the
 * entry points reject. */
size_t mr_carafe_backward_workspace_bytes(int n, int channels, int h, int w, int up_kernel, int up_group, int scale_factor);

/*
 * mr_carafe_pack_backward: the gradients of mr_carafe_pack_forward's out to x (the reassembly's direct path; the path through m is the
 * caller's, through grad_m) and to m, in m's layout, from x, m and grad_out (n, channels, h s, w s) alone: the softmax is recomputed.  At most
 * TWO launches, no atomics: bitwise reproducible, and a RoI's gradients do not depend on the batch.
 *   launch 1 (when grad_m or grad_x is wanted): per output pixel and group  gw_t = sum_{c in g} grad_out[c] x[c, window t]  — one workgroup
 *     walks all the group's channels in order, one fma chain per thread —, then  grad_m[.. t ..] = w_t (gw_t - sum_t w_t gw_t)  at the logit's
 *     place in m (the inverse shuffle; every element of grad_m is written), and w_t to the workspace when grad_x is wanted;
 *   launch 2 (when grad_x is wanted): grad_x[c, y, x] = sum_{dy, dx < s} sum_t grad_out[c, (y - iy + r) s + dy, (x - ix + r) s + dx]
 *     w_t[the same output pixel], a gather in the order (dy, dx), then t, over the output pixels whose window covers (y, x).
 * grad_x (x's shape) and grad_m (m's shape) may each be NULL (not wanted); workspace (mr_carafe_backward_workspace_bytes, 4-byte aligned) may
 * be NULL when grad_x is.  Errors as mr_carafe_pack_forward; MR_ERR_BAD_ARGUMENT for a workspace that is too small.
 */
int mr_carafe_pack_backward(const float *x, const float *m, const float *grad_out, int n, int channels, int h, int w, int up_kernel,
                            int up_group, int scale_factor, void *workspace, size_t workspace_bytes, float *grad_x, float *grad_m,
                            void *stream);

#ifdef __cplusplus
}
#endif
#endif
