/*
 * monorun_global.h — C ABI of the global head of libmonorun_pnp.so: the Monte-Carlo dropout extractor in front of the NOC decode and the
 * score head.  The entry points are compiled into the same library as those of monorun_pnp.h and follow the conventions of
 * monorun_heads.h: 0 on success or a negative MR_ERR_* code of monorun_pnp.h; every data pointer is a DEVICE pointer, dereferenced only
 * by the kernels, in stream order; a call runs on the current HIP device, asynchronously on `stream`; nothing is allocated.
 *
 * Reference interface replaced: FCExtractorMonteCarlo.forward of the MonoRUn tree in eval mode
 * (monorun/models/roi_heads/bbox_3d_heads/global_extractors/fc_extractor_monte_carlo.py:41-63 over fc_extractor.py:93-107) with
 * num_fcs = 2 and num_dropout_layers = 2, the dropout draws given by the caller as masks.
 */
#ifndef MONORUN_GLOBAL_H_
#define MONORUN_GLOBAL_H_

#include <stddef.h>
#include <stdint.h>
#include "monorun_pnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* limits of mr_global_head_mc_forward; beyond them MR_ERR_UNSUPPORTED */
#define MR_GLOBAL_MAX_CHANNELS 8192        /* in_channels, area and fc_channels, each */
#define MR_GLOBAL_MAX_OUT 4096             /* out_channels */
#define MR_GLOBAL_MAX_SAMPLES 4096         /* num_samples */
#define MR_GLOBAL_CHUNK 64                 /* RoIs per pass: what bounds the workspace */

/*
 * mr_global_head_mc_forward: with C = in_channels, A = area (rh * rw), F = fc_channels, J = out_channels, S = num_samples, for RoI
 * i < n, sample s < S (sample row s * n + i: the layout of x.repeat(S, 1, 1, 1) and of view(S, -1, J)):
 *   P[i,c,o]   = sum_{k<A} x[i,c,k] * W1[o, c*A + k]                                                 once per RoI
 *   h1[s,i,o]  = k1 * relu(b1[o] + q0 * sum_{c<C} m0[s,i,c] * P[i,c,o])      m0 = keep0 ? 1 : 0,  k1 = keep1[s,i,o] ? q1 : 0
 *   h2[s,i,o]  = k2 * relu(b2[o] + sum_{k<F} W2[o,k] * h1[s,i,k])                                 k2 = keep2[s,i,o] ? q1 : 0
 *   y[s,i,j]   = bR[j] + sum_{k<F} WR[j,k] * h2[s,i,k]
 *   mean[i,j]  = (sum_s y[s,i,j]) / S
 *   var[i,j]   = (sum_s (y[s,i,j] - mean)^2) / (S - 1)                          two passes, the mean unrounded
 *   reg_fc_out[i,k] = (sum_s h2[s,i,k]) / S
 *   samples[s,i,j]  = y[s,i,j]                                                  when `samples` is not NULL
 * which is W1 (x * m0 * q0) of dropout2d factored over the channel mask: the S samples of a RoI share P.  q0 = 1 / (1 - dropout2d
 * rate) and q1 = 1 / (1 - dropout rate) are the caller's.  fp32 throughout, every sum over c or k one fused-multiply-add chain in
 * ascending index (the output layer: 64 interleaved chains, then fp64 adds in a fixed order); the three sums over s are fp64 and each
 * result is rounded to fp32 once.  relu keeps NaN, as torch's does, and NaN * 0 of a dropped element stays NaN.  No split of a sum
 * across workgroups and no floating-point atomics: the order of every sum depends on C, A, F, J and S only, so a RoI's results are
 * bitwise the same alone and anywhere in a batch, given its own masks, and two calls agree bitwise.
 *
 * Inputs, device, contiguous, fp32 unless stated:
 *   x (n, C, A);  w1 (F, C*A), b1 (F);  w2 (F, F), b2 (F);  w_reg (J, F), b_reg (J): nn.Linear's own layout, nothing is repacked;
 *   keep0 (S, n, C), keep1 (S, n, F), keep2 (S, n, F): uint8_t (torch.bool memory), non-zero = kept.
 * Outputs: mean (n, J), var (n, J), reg_fc_out (n, F); samples (S, n, J) or NULL.
 * workspace: at least mr_global_head_mc_workspace_bytes(...) bytes, 4-byte aligned, the caller's; it holds P, h1, h2 and y of one
 *   pass of min(n, MR_GLOBAL_CHUNK) RoIs — 4 * min(n, MR_GLOBAL_CHUNK) * (C*F + 2*S*F + S*J) bytes — is fully written before it is
 *   read, and its contents before and after a call mean nothing.  RoIs beyond MR_GLOBAL_CHUNK are processed pass after pass
 *   inside the one call.
 *
 * n = 0 launches nothing and returns 0.  MR_ERR_BAD_ARGUMENT, before any HIP call, for a negative n, a size below 1, S < 2, a NULL
 * required pointer (all but samples and stream) or a workspace_bytes below the required size.  MR_ERR_UNSUPPORTED for C, A or F above
 * MR_GLOBAL_MAX_CHANNELS, J above MR_GLOBAL_MAX_OUT, S above MR_GLOBAL_MAX_SAMPLES, or when one of the products n*C*A, F*C*A,
 * S*n*F, S*n*C or S*n*J exceeds 2^31 - 1 (element counts of the tensors are kept in 32 bits by callers of this library).
 * mr_global_head_mc_workspace_bytes returns 0 for arguments the forward call would reject, and for n = 0.
 */
size_t mr_global_head_mc_workspace_bytes(int n, int in_channels, int area, int fc_channels, int out_channels, int num_samples);

int mr_global_head_mc_forward(const float *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *w_reg,
                              const float *b_reg, const uint8_t *keep0, const uint8_t *keep1, const uint8_t *keep2, float q0, float q1,
                              int n, int in_channels, int area, int fc_channels, int out_channels, int num_samples, void *workspace,
                              size_t workspace_bytes, float *mean, float *var, float *reg_fc_out, float *samples, void *stream);

#ifdef __cplusplus
}
#endif
#endif
