// monorun_pnp.hip — gfx950 (MI355X / CDNA4) kernels + C ABI for MonoRUn's uncertainty-aware PnP hot path.
// One translation unit: this file holds the includes, the compile-time switches, the fused kernel's argument blocks and two lists of
// includes.  The kernels live in the *_kernel.inc files (the fused per-object kernel: pnp_kernel.inc; K2: noc_decode_kernel.inc; RoIAlign,
// NMS and the eigenvalue rule: consumers_kernel.inc), the host side of the launches in host_launch.inc, and the C ABI (the entry points the
// headers under include/ declare, in the headers' order) in the *_abi.inc files, one per header.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <map>
#include <utility>
#include <stdlib.h>
#include <vector>
#include <type_traits>

#include "monorun_pnp.h"
#include "monorun_heads.h"
#include "monorun_train.h"
#include "monorun_targets.h"
#include "monorun_global.h"
#include "monorun_carafe.h"
#include "monorun_roi.h"
#include "monorun_proposals.h"
#include "monorun_bbox.h"
#include "monorun_assign.h"
#include "monorun_fpn.h"
#include "monorun_backbone.h"
#include "monorun_result3d.h"
#include "monorun_roi_train.h"
#include "monorun_image.h"

namespace {

constexpr int kMaxLeaves = 64;      // numpy pairwise-sum leaves (blocks of <=128) supported per object
constexpr int kMaxChunks = 128;     // 64-point chunks per object (P <= 8192; LDS caps P well below that)
constexpr int kHyp = 32;            // K0 hypotheses (the reference's RANSAC runs 30 iterations)
constexpr uint32_t kK0Seed = 0x9E3779B9u;
constexpr int kRedN = 32;           // doubles per wave in the cross-wave reduction scratch
constexpr int kMaxDevices = 64;     // per-device library state (LDS opt-in, host-entry staging) is keyed by HIP device id
#ifndef MR_MIN_WAVES
#define MR_MIN_WAVES 3              // waves per SIMD the register allocator must allow: fp64 storage (<= 168 VGPRs)
#endif
#ifndef MR_RELAXED_WPO
#define MR_RELAXED_WPO 2            // instantiations with at most this many waves per object are compiled for 3 waves per SIMD (168 VGPRs):
                                    // they serve large batches, where LDS allows 5 workgroups = 10 waves per CU anyway; 8192-object launch 297 -> 289 us
#endif
#ifndef MR_MIN_WAVES_F32
#define MR_MIN_WAVES_F32 4          // fp32 and 16-bit storage (the pipeline's cases): <= 128 VGPRs, so that the 1024 four-wave blocks of a
#endif                              // config-2 launch are all resident (measured: 76 us vs 83 us when the allocator lands on 139 VGPRs)

#include "noc_decode_kernel.inc"

// numpy's pairwise summation tree for a length-P contiguous float32 reduction, built on the host:
// leaves (blocks of <=128 elements) + the combine tree, internal nodes ordered by height so that the
// kernel can evaluate it level by level.  Value slots: [0, n_leaves) leaves, n_leaves + k internal k.
struct PairwisePlan {
    int n_leaves, n_internal, n_levels, root;
    uint16_t leaf_off[kMaxLeaves];
    uint16_t leaf_len[kMaxLeaves];
    uint8_t left[kMaxLeaves], right[kMaxLeaves];
    uint8_t level_start[16];
};

struct PnpArgs {
    const void *x2d, *istd, *x3d;
    long long s2[3], sw[3], s3[3];            // global element strides (b, p, c)
    int vec;                                   // 1: point stride 1 on all three tensors (channel-planar rows): load_records' coalesced path
    int elem_size;                             // sizeof(T) of the correspondence tensors
    int nca, nla;                              // LDS carve: chunk slots (multiple of 4), pairwise leaves (>= 1)
    const void *K; int K_stride; int K_f64;    // K_stride 0 (broadcast) or 9
    const void *ur, *vr; int r_stride; int r_f64;
    const float *ransac_thr;
    const double *init_pose;
    int B, P;
    double z_min; float istd_thres; int inlier_opt_only; int flags; int mean_mode;
    int lm_max_iter;                           // Ceres max_num_iterations (50 unless MR_LM_MAXIT bits are set)
    uint8_t *valid; float *pose; float *cov; float *tr; uint8_t *mask; float *diag;
    double *pose64, *cov64, *tr64;            // legacy per-object ABI outputs (nullable)
    unsigned long long *stamps;               // debug: (B,24) s_memtime stamps (nullable)
    const float *calib_logscale; float corr_sd; float *cov_calib;   // optional fused R8/R13 epilogue: calibrated + distance-corrected covariance
    int from_head;                            // 1: the tile is decoded in-kernel from the raw NOC-head output (`dec`)
    DecodeArgs dec;
    PairwisePlan plan;
    const uint8_t *init_mask, *init_valid;    // EXT launches only (appended: the offsets of everything above are what the tuned kernels read)
};
// EXT launches over the objects of several calls (mr_pnp_uncert_from_init_grouped; a SECOND kernel argument of a kernel of its own, so that
// the argument block — and with it the code — of every other instantiation stays what it was): object b belongs to call b / group_B, whose
// pointers — biased on the host so that the GLOBAL object index addresses them — replace PnpArgs'
struct PnpCallTable {
    int ncalls, group_B;
    struct CallPtrs {
        const void *x2d, *istd, *x3d, *K, *ur, *vr;
        const double *init_pose; const uint8_t *init_mask, *init_valid;
        uint8_t *valid; float *pose, *cov, *tr; uint8_t *mask; float *diag; float *cov_calib;
    } call[8];          // = kEpMaxGroup
};

#include "pnp_kernel.inc"
#include "pnp6_kernel.inc"
#include "hessian_kernel.inc"
#include "pnp_backward_kernel.inc"
#include "pnp_noc_kernel.inc"
#include "epnp_kernel.inc"
#include "epnp_eig_low4.inc"
#include "epnp_stages.inc"
constexpr size_t kNocLds = sizeof(double) * (2 * 4 * kRedN + 2 * 40);     // reduction scratch + two sets of block sums
#include "kitti_eval_kernel.inc"
#include "iou3d_kernel.inc"
#include "projection_loss_kernel.inc"
#include "noc_decode_train_kernel.inc"
#include "noc_target_kernel.inc"
#include "score_head_kernel.inc"
#include "global_head_kernel.inc"
#include "carafe_kernel.inc"
#include "roi_extract_kernel.inc"
#include "proposals_kernel.inc"
#include "bbox_head_kernel.inc"
#include "assign_kernel.inc"
#include "fpn_kernel.inc"
#include "backbone_kernel.inc"
#include "consumers_kernel.inc"
#include "result3d_kernel.inc"
#include "roi_train_kernel.inc"
#include "image_prepare_kernel.inc"
#include "host_launch.inc"

}  // namespace

// ================================================================================= C ABI =========
// The host side of every entry point, one file per public header in the order the headers are included above (monorun_pnp.h's share by
// the header's sections), then the development aids no header declares.
extern "C" {

#include "pnp_library_abi.inc"
#include "pnp_solver_abi.inc"
#include "pnp_host_abi.inc"
#include "pnp_decode_abi.inc"
#include "pnp_losses_abi.inc"
#include "pnp_eval_abi.inc"
#include "heads_abi.inc"
#include "train_abi.inc"
#include "targets_abi.inc"
#include "global_abi.inc"
#include "carafe_abi.inc"
#include "roi_extract_abi.inc"
#include "proposals_abi.inc"
#include "bbox_head_abi.inc"
#include "assign_abi.inc"
#include "fpn_abi.inc"
#include "backbone_abi.inc"
#include "result3d_abi.inc"
#include "roi_train_abi.inc"
#include "image_abi.inc"
#include "debug_abi.inc"

}  // extern "C"
