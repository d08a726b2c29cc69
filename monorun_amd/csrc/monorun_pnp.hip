// monorun_pnp.hip — gfx950 (MI355X / CDNA4) kernels + C ABI for MonoRUn's uncertainty-aware PnP hot path.
// One translation unit: this file holds the includes, the compile-time switches, the kernel argument blocks and the C ABI (declared in
// include/monorun_pnp.h, monorun_heads.h and monorun_train.h, defined here in the headers' order); the kernels live in the *_kernel.inc files (the fused
// per-object kernel: pnp_kernel.inc; K2: noc_decode_kernel.inc; RoIAlign, NMS and the eigenvalue rule: consumers_kernel.inc), the
// host side of the launches in host_launch.inc.
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
#include "consumers_kernel.inc"
#include "host_launch.inc"

}  // namespace

// ================================================================================= C ABI =========
extern "C" {

int mr_pnp_version(void) { return MR_PNP_VERSION; }

const char *mr_pnp_error_string(int code) {
    switch (code) {
        case MR_OK: return "ok";
        case MR_ERR_BAD_ARGUMENT: return "bad argument";
        case MR_ERR_UNSUPPORTED: return "unsupported configuration (P too large for LDS, or unknown dtype)";
        case MR_ERR_HIP: return "HIP runtime error (see mr_pnp_last_hip_error)";
        case MR_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown error";
    }
}

int mr_pnp_last_hip_error(void) { return g_last_hip_error; }

int mr_pnp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// waves per object the library would pick for a launch of `objects_in_flight` objects x P points on the current device (pick_wpo): lets
// a caller that keeps several launches in flight apply the library's own rule to ALL the objects on the chip (PnPPipeline.flags_for)
int mr_pick_waves(int objects_in_flight, int P) {
    if (objects_in_flight < 1 || P < 4) return MR_ERR_BAD_ARGUMENT;
    return pick_wpo(objects_in_flight, P, 0);
}

// Occupies one wavefront of the device for `microseconds` (100 MHz constant clock).  PnPPipeline uses it to find out which of
// its streams the runtime really runs side by side: HIP maps streams onto a small number of hardware queues (4 per priority level
// by default) and two streams that share a queue serialise.
int mr_spin(int microseconds, void *stream) {
    if (microseconds < 0 || microseconds > 1000000) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)microseconds * 100);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

static int pnp_uncert_launch(
    const CorrIn &in, int in_dtype,
    const float *ransac_thr, const double *init_pose, const uint8_t *init_mask, const uint8_t *init_valid, int B, int P,
    float z_min, float istd_thres, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag, void *stream,
    int ncalls = 1, const PnpCallTable::CallPtrs *calls = nullptr, const EpnpRefitIn *rf = nullptr, const float *calib_logscale = nullptr, float corr_sd = 0.0f) {
    if (B < 0 || P < 4 || P > 64 * kMaxChunks) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !valid || !pose || !tr_radius || (!cov && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    PnpArgs a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.ransac_thr = ransac_thr; a.init_pose = init_pose; a.init_mask = init_mask; a.init_valid = init_valid;
    a.B = B; a.P = P; a.z_min = (double)z_min; a.istd_thres = istd_thres; a.inlier_opt_only = inlier_opt_only; a.flags = flags;
    a.valid = valid; a.pose = pose; a.cov = cov; a.tr = tr_radius; a.mask = inlier_mask; a.diag = diag;
    a.stamps = g_stamps;
    if (calib_logscale && calls && calls[0].cov_calib) { a.calib_logscale = calib_logscale; a.corr_sd = corr_sd; a.cov_calib = calls[0].cov_calib; }      // per call: the table's
    int rc;
    if ((rc = choose_mean_order(a)) != MR_OK) return rc;
    PnpCallTable tbl;
    memset(&tbl, 0, sizeof tbl);
    tbl.ncalls = 1; tbl.group_B = B;
    if (ncalls > 1 || rf) {                             // a launch over the objects of several calls (EXT only): mr_pnp_uncert_from_init_grouped / _from_epnp_grouped
        tbl.ncalls = ncalls; a.B = B * ncalls;
        for (int c = 0; c < ncalls; ++c) tbl.call[c] = calls[c];
    }
    const int wpo = lm_launch_waves(a, flags, in_dtype);
    hipStream_t st = (hipStream_t)stream;
    const PnpCallTable *tp = (ncalls > 1 || rf) ? &tbl : nullptr;
    return with_storage_type(in_dtype, [&](auto t) { return launch_wpo<typename decltype(t)::type>(a, wpo, st, tp, rf); });
}

int mr_pnp_uncert_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const float *ransac_thr, const double *init_pose, int B, int P,
    float z_min, float istd_thres, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag, void *stream) {
    return pnp_uncert_launch({ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch }, in_dtype,
                             ransac_thr, init_pose, nullptr, nullptr, B, P, z_min, istd_thres, inlier_opt_only, flags,
                             valid, pose, cov, tr_radius, inlier_mask, diag, stream);
}

static int epnp_ransac_launch(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *ransac_thr, int B, int P,
    float istd_thres, int flags, int max_iters,
    double *const *init_pose, uint8_t *const *init_mask, uint8_t *const *init_valid, float *const *diag, double *debug_hypotheses,
    void *workspace, size_t workspace_bytes, void *stream) {
    if (ncalls < 1 || ncalls > kEpMaxGroup || B < 0 || P < 4 || P > 64 * kMaxChunks || max_iters < 1 || max_iters > kEpMaxIters) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if ((long long)B * ncalls > 0x7fffffffll / kEpMaxIters) return MR_ERR_UNSUPPORTED;
    if (!x2d || !istd || !x3d || !x2d_strides || !istd_strides || !x3d_strides || !cam_mats || !init_pose || !init_mask || !init_valid) return MR_ERR_BAD_ARGUMENT;
    const CorrIn in{ x2d[0], x2d_strides, istd[0], istd_strides, x3d[0], x3d_strides, cam_mats[0], cam_batch, nullptr, nullptr, 1 };
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    EpnpStageArgs sa;
    memset(&sa, 0, sizeof sa);
    for (int c = 0; c < ncalls; ++c) {
        if (!x2d[c] || !istd[c] || !x3d[c] || !cam_mats[c] || !init_pose[c] || !init_mask[c] || !init_valid[c]) return MR_ERR_BAD_ARGUMENT;
        const CallBias at(c, B, in_dtype);
        if (at.mixed(ransac_thr) || at.mixed(diag)) return MR_ERR_BAD_ARGUMENT;     // all or none
        EpnpCallPtrs &q = sa.call[c];
        q.x2d = at(x2d, x2d_strides); q.istd = at(istd, istd_strides); q.x3d = at(x3d, x3d_strides); q.K = at(cam_mats, cam_batch == 1 ? 0 : 9);
        q.ransac_thr = at(ransac_thr, 1);
        q.init_pose = at(init_pose, 4); q.init_mask = at(init_mask, P); q.init_ok = at(init_valid, 1); q.diag = at(diag, 4);
    }
    if (debug_hypotheses && ncalls != 1) return MR_ERR_BAD_ARGUMENT;
    if ((flags & MR_EPNP_DEFER_REFIT) && !workspace) return MR_ERR_BAD_ARGUMENT;       // the LM launch that finishes the job needs the workspace
    PnpArgs &a = sa.p;
    set_inputs(a, in);
    a.ransac_thr = ransac_thr ? ransac_thr[0] : nullptr;
    a.B = B * ncalls; a.P = P; a.istd_thres = istd_thres; a.flags = flags;
    int rc;
    if ((rc = choose_mean_order(a)) != MR_OK) return rc;
    a.stamps = g_stamps;
#ifdef MR_DEBUG_STAMPS
    sa.cstamps = g_cons_stamps;
#endif
    sa.init_pose = init_pose[0]; sa.init_mask = init_mask[0]; sa.init_ok = init_valid[0]; sa.diag = diag ? diag[0] : nullptr; sa.dbg_hyp = debug_hypotheses; sa.max_iters = max_iters;
    sa.ncalls = ncalls; sa.group_B = B;
    hipStream_t st = (hipStream_t)stream;
    // hypotheses solved for every object before the replayed loop is consulted: MR_EPNP_FIRST_ROUND bits of `flags` (1..30), else the
    // environment variable MR_EPNP_FIRST_ROUND, else by the size of the launch set: 10 up to 2047 objects (one call at a time: the
    // second round is a full latency chain; 8 hypotheses make it idle in 85 % of config-2 batches, 10 in 97 %: 278.6 -> 264.1 us per
    // 1024-object call, 228.9 -> 221.8 at 256, within noise at 100 — profiles/r06_first_round.txt), 3 beyond (several calls grouped
    // or a large batch: the chip is busy, the hypotheses nobody needs are the cost — sets of three calls: 9.6 / 9.9 / 10.3 / 10.3 M solves/s
    // with 6 / 4 / 3 / 2, profiles/r05_epnp_grouped_first_round.txt).  Changes the work, never a result.
    static const int first_env = [] { const char *e = getenv("MR_EPNP_FIRST_ROUND"); const int v = e ? atoi(e) : 0; return v < 1 ? 0 : (v > 30 ? 30 : v); }();
    const int first_bits = (flags & MR_EPNP_FIRST_ROUND_MASK) >> MR_EPNP_FIRST_ROUND_SHIFT;
    const int first_round = first_bits ? (first_bits > 30 ? 30 : first_bits) : (first_env ? first_env : ((long long)B * ncalls >= 2048 ? 3 : 10));
    return with_storage_type(in_dtype, [&](auto t) { return launch_epnp_stages<typename decltype(t)::type>(sa, workspace, workspace_bytes, first_round, st); });
}

int mr_epnp_ransac_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *ransac_thr, int B, int P,
    float istd_thres, int flags, int max_iters,
    double *init_pose, uint8_t *init_mask, uint8_t *init_valid, float *diag, double *debug_hypotheses,
    void *workspace, size_t workspace_bytes, void *stream) {
    return epnp_ransac_launch(1, &x2d, x2d_strides, &istd, istd_strides, &x3d, x3d_strides, in_dtype, &cam_mats, cam_batch, &ransac_thr, B, P,
                              istd_thres, flags, max_iters, &init_pose, &init_mask, &init_valid, &diag, debug_hypotheses, workspace, workspace_bytes, stream);
}

size_t mr_epnp_workspace_bytes(int B, int P) {
    if (B <= 0 || P < 4) return 0;
    return epnp_work_bytes(B, P, nullptr, nullptr);
}

int mr_epnp_ransac_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *ransac_thr, int B, int P,
    float istd_thres, int flags, int max_iters,
    double *const *init_pose, uint8_t *const *init_mask, uint8_t *const *init_valid, float *const *diag,
    void *workspace, size_t workspace_bytes, void *stream) {
    return epnp_ransac_launch(ncalls, x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, in_dtype, cam_mats, cam_batch, ransac_thr, B, P,
                              istd_thres, flags, max_iters, init_pose, init_mask, init_valid, diag, nullptr, workspace, workspace_bytes, stream);
}

int mr_pnp_uncert_from_init_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const double *init_pose, const uint8_t *init_mask, const uint8_t *init_valid, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag, void *stream) {
    if (B > 0 && (!init_pose || !init_mask || !init_valid)) return MR_ERR_BAD_ARGUMENT;
    return pnp_uncert_launch({ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch }, in_dtype,
                             nullptr, init_pose, init_mask, init_valid, B, P, z_min, 0.0f, inlier_opt_only, flags,
                             valid, pose, cov, tr_radius, inlier_mask, diag, stream);
}

static int pnp_from_init_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *u_range, const float *const *v_range, int range_batch,
    const double *const *init_pose, const uint8_t *const *init_mask, const uint8_t *const *init_valid, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *const *valid, float *const *pose, float *const *cov, float *const *tr_radius, uint8_t *const *inlier_mask, float *const *diag, void *stream,
    EpnpRefitIn *rf = nullptr, float *const *epnp_diag = nullptr, const float *calib_logscale = nullptr, float corr_sd = 0.0f, float *const *cov_calib = nullptr) {
    if (ncalls < 1 || ncalls > 8 || B < 0) return MR_ERR_BAD_ARGUMENT;
    const bool with_calib = cov_calib && cov_calib[0];
    if (with_calib && (!calib_logscale || (flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!x2d || !istd || !x3d || !x2d_strides || !istd_strides || !x3d_strides || !cam_mats || !u_range || !v_range || !init_pose || !init_mask || !init_valid ||
        !valid || !pose || !tr_radius || (!cov && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;       // (no covariance asked: the table itself may be NULL, like its entries)
    if ((long long)B * ncalls > 0x7fffffffll / kEpMaxIters) return MR_ERR_UNSUPPORTED;                         // objects are numbered through the set in int arithmetic (as in epnp_ransac_launch)
    const long long ks = (cam_batch == 1) ? 0 : 9, rs = (range_batch == 1) ? 0 : 2;
    PnpCallTable::CallPtrs cp[8];
    for (int c = 0; c < ncalls; ++c) {
        if (!x2d[c] || !istd[c] || !x3d[c] || !cam_mats[c] || !u_range[c] || !v_range[c] || !init_pose[c] || !init_mask[c] || !init_valid[c] ||
            !valid[c] || !pose[c] || !tr_radius[c] || (!(cov && cov[c]) && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
        const CallBias at(c, B, in_dtype);
        if (at.mixed(inlier_mask) || at.mixed(diag) || at.mixed(cov_calib)) return MR_ERR_BAD_ARGUMENT;       // all or none
        PnpCallTable::CallPtrs &q = cp[c];
        q.x2d = at(x2d, x2d_strides); q.istd = at(istd, istd_strides); q.x3d = at(x3d, x3d_strides);
        q.K = at(cam_mats, ks); q.ur = at(u_range, rs); q.vr = at(v_range, rs);
        q.init_pose = at(init_pose, 4); q.init_mask = at(init_mask, P); q.init_valid = at(init_valid, 1);
        q.valid = at(valid, 1); q.pose = at(pose, 4); q.cov = at(cov, 16); q.tr = at(tr_radius, 1);
        q.mask = at(inlier_mask, P); q.diag = at(diag, 4); q.cov_calib = at(cov_calib, 16);
        if (rf) rf->diag[c] = at(epnp_diag, 4);
    }
    return pnp_uncert_launch({ x2d[0], x2d_strides, istd[0], istd_strides, x3d[0], x3d_strides, cam_mats[0], cam_batch, u_range[0], v_range[0], range_batch },
                             in_dtype, nullptr, init_pose[0], init_mask[0], init_valid[0], B, P, z_min, 0.0f, inlier_opt_only, flags,
                             valid[0], pose[0], cov ? cov[0] : nullptr, tr_radius[0], inlier_mask ? inlier_mask[0] : nullptr, diag ? diag[0] : nullptr, stream,
                             ncalls, cp, rf, calib_logscale, corr_sd);
}

int mr_pnp_uncert_from_init_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *u_range, const float *const *v_range, int range_batch,
    const double *const *init_pose, const uint8_t *const *init_mask, const uint8_t *const *init_valid, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *const *valid, float *const *pose, float *const *cov, float *const *tr_radius, uint8_t *const *inlier_mask, float *const *diag, void *stream) {
    return pnp_from_init_grouped(ncalls, x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, in_dtype, cam_mats, cam_batch, u_range, v_range, range_batch,
                                 init_pose, init_mask, init_valid, B, P, z_min, inlier_opt_only, flags, valid, pose, cov, tr_radius, inlier_mask, diag, stream);
}

int mr_pnp_uncert_from_epnp_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *u_range, const float *const *v_range, int range_batch,
    double *const *init_pose, const uint8_t *const *init_mask, uint8_t *const *init_valid, float *const *epnp_diag, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *const *valid, float *const *pose, float *const *cov, float *const *tr_radius, uint8_t *const *inlier_mask, float *const *diag,
    const float *cov_calib_logscale, float cov_corr_sd, float *const *cov_calib,
    const void *workspace, size_t workspace_bytes, void *stream) {
    if (ncalls < 1 || ncalls > kEpMaxGroup || B < 0 || P < 4) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if ((long long)B * ncalls > 0x7fffffffll / kEpMaxIters) return MR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < epnp_work_bytes(B * ncalls, P, nullptr, nullptr)) return MR_ERR_BAD_ARGUMENT;
    EpnpRefitIn rf;
    memset(&rf, 0, sizeof rf);
    epnp_work_bytes(B * ncalls, P, &rf.w, (unsigned char *)const_cast<void *>(workspace));
    rf.B = (long long)B * ncalls;
    return pnp_from_init_grouped(ncalls, x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, in_dtype, cam_mats, cam_batch, u_range, v_range, range_batch,
                                 (const double *const *)init_pose, init_mask, (const uint8_t *const *)init_valid, B, P, z_min, inlier_opt_only, flags,
                                 valid, pose, cov, tr_radius, inlier_mask, diag, stream, &rf, epnp_diag, cov_calib_logscale, cov_corr_sd, cov_calib);
}

int mr_cov_symeig_rule(uint8_t *valid, float *cov, int B, float *eig_min_max, void *stream) {
    if (B < 0) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!valid || !cov) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(cov_symeig_rule_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, valid, cov, B, eig_min_max);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_pnp6_refine_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const uint8_t *inlier_mask, const float *pose4, const uint8_t *valid4, int B, int P, float z_min, int flags,
    uint8_t *valid, float *pose6, float *cov6, float *diag, void *stream) {
    const CorrIn in{ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (B < 0 || P < 4 || P > 64 * kMaxChunks) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !inlier_mask || !pose4 || !valid4 || !valid || !pose6 || !cov6) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    Pnp6Args a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.mask = inlier_mask; a.pose4 = pose4; a.valid4 = valid4;
    a.B = B; a.P = P; a.z_min = (double)z_min; a.lm_max_iter = lm_max_iter(flags);
    a.valid = valid; a.pose6 = pose6; a.cov6 = cov6; a.diag = diag;
    return with_storage_type(in_dtype, [&](auto t) { return launch_pnp6<typename decltype(t)::type>(a, (hipStream_t)stream); });
}

int mr_pnp_exact_hessian_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const float *pose, const uint8_t *inlier_mask, int B, int P, float z_min,
    uint8_t *valid, float *hess, float *cov, void *stream) {
    const CorrIn in{ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (B < 0 || P < 1) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !pose || !valid || !cov) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    HessArgs a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.pose = pose; a.mask = inlier_mask; a.B = B; a.P = P; a.z_min = (double)z_min;
    a.valid = valid; a.hess = hess; a.cov = cov;
    return with_storage_type(in_dtype, [&](auto t) {
        hipLaunchKernelGGL((exact_hessian_kernel<typename decltype(t)::type>), dim3(B), dim3(256), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    });
}

int mr_pnp_uncert_backward_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const float *pose, const uint8_t *inlier_mask, const uint8_t *valid, int lm_all_points,
    const float *grad_pose, const float *cov, const float *grad_cov, int B, int P, float z_min,
    float *grad_x2d, float *grad_istd, float *grad_x3d, uint8_t *status, void *stream) {
    const CorrIn in{ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (B < 0 || P < 1) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !pose || !valid) return MR_ERR_BAD_ARGUMENT;
    if ((cov == nullptr) != (grad_cov == nullptr)) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    PnpBwdArgs a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.pose = pose; a.mask = inlier_mask; a.valid = valid; a.lm_all = lm_all_points ? 1 : 0;
    a.grad_pose = grad_pose; a.cov = cov; a.grad_cov = grad_cov;
    a.B = B; a.P = P; a.z_min = (double)z_min;
    a.g2 = grad_x2d; a.gw = grad_istd; a.g3 = grad_x3d; a.status = status;
    return with_storage_type(in_dtype, [&](auto t) {
        hipLaunchKernelGGL((pnp_uncert_backward_kernel<typename decltype(t)::type>), dim3(B), dim3(256), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    });
}

// ---- host-buffer entry points of the reference's C ABI (ext.h).  Per device: one private non-blocking stream, one pinned
// host staging buffer and one device buffer, grown on demand and kept; a call is one async H2D copy, the kernel and one async
// D2H copy on that stream followed by a single hipStreamSynchronize (no default-stream launch, no pageable copies, no
// allocation in the steady state).  Calls on the same device serialise on the stage's mutex (the reference invokes these
// serially, pnp_uncert_cpu.py:180-191); calls on different devices run concurrently.
struct HostStage {
    std::mutex mu;
    hipStream_t st = nullptr;
    void *dbuf = nullptr, *hbuf = nullptr;
    size_t cap = 0;
};
static HostStage g_stage[kMaxDevices];

// returns the locked stage of the current device with room for `bytes` in both buffers, or nullptr (lock not held)
static HostStage *stage_acquire(size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { g_last_hip_error = (int)hipGetLastError(); return nullptr; }
    HostStage *s = &g_stage[dev];
    s->mu.lock();
    bool ok = true;
    if (!s->st) ok = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) == hipSuccess;
    if (ok && bytes > s->cap) {
        const size_t want = bytes < 4096 ? 4096 : bytes + bytes / 2;
        if (s->dbuf) (void)hipFree(s->dbuf);
        if (s->hbuf) (void)hipHostFree(s->hbuf);
        s->dbuf = s->hbuf = nullptr; s->cap = 0;
        ok = hipMalloc(&s->dbuf, want) == hipSuccess && hipHostMalloc(&s->hbuf, want, hipHostMallocDefault) == hipSuccess;
        if (ok) s->cap = want;
    }
    if (!ok) { g_last_hip_error = (int)hipGetLastError(); s->mu.unlock(); return nullptr; }
    return s;
}

// The reference's per-object entry point (ext.h:1-13).  Host fp64 buffers; one object; blocking.
void pnp_uncert(double *pts2d, double *pts3d, double *wgt2d, double *K, double *init_pose,
                int *result_val, double *result_pose, double *result_cov, double *result_tr,
                int pn, double *clips) {
    *result_val = 0;
    memcpy(result_pose, init_pose, 4 * sizeof(double));                  // pnp_uncert_cpu.cpp:259
    *result_tr = 0.0;
    if (pn < 1 || pn > 65535) return;
    const int P = pn < 4 ? 4 : pn;
    // staging, in doubles: [pts2d 2P | pts3d 3P | wgt 2P | K 9 | ur 2 | vr 2 | init 4 || pose64 4 | cov64 16 | tr64 1 | valid (u8, 8 bytes)]
    //                      + [pose 4 | cov 16 | tr 1] floats (written by the kernel, not read back)
    const size_t nin = (size_t)7 * P + 9 + 2 + 2 + 4, nout = 4 + 16 + 1 + 1;
    const size_t bytes = (nin + nout) * sizeof(double) + 24 * sizeof(float);
    HostStage *sg = stage_acquire(bytes);
    if (!sg) return;
    std::lock_guard<std::mutex> lk(sg->mu, std::adopt_lock);
    double *h = (double *)sg->hbuf, *d = (double *)sg->dbuf;
    double *h2 = h, *h3 = h2 + 2 * P, *hw = h3 + 3 * P, *hK = hw + 2 * P, *hur = hK + 9, *hvr = hur + 2, *hin = hvr + 2;
    memcpy(h2, pts2d, sizeof(double) * 2 * pn); memcpy(h3, pts3d, sizeof(double) * 3 * pn); memcpy(hw, wgt2d, sizeof(double) * 2 * pn);
    for (int p = pn; p < P; ++p) { h2[2 * p] = h2[2 * p + 1] = 0.0; h3[3 * p] = h3[3 * p + 1] = 0.0; h3[3 * p + 2] = 1.0; hw[2 * p] = hw[2 * p + 1] = 0.0; }   // padded points carry zero weight
    memcpy(hK, K, sizeof(double) * 9);
    hur[0] = clips[1]; hur[1] = clips[2]; hvr[0] = clips[3]; hvr[1] = clips[4];
    memcpy(hin, init_pose, sizeof(double) * 4);
    if (hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    PnpArgs a;
    memset(&a, 0, sizeof a);
    a.x2d = d; a.x3d = d + 2 * P; a.istd = d + 5 * P;
    a.s2[0] = 0; a.s2[1] = 2; a.s2[2] = 1; a.sw[0] = 0; a.sw[1] = 2; a.sw[2] = 1; a.s3[0] = 0; a.s3[1] = 3; a.s3[2] = 1;
    a.K = d + 7 * P; a.K_stride = 0; a.K_f64 = 1;
    a.ur = d + 7 * P + 9; a.vr = d + 7 * P + 11; a.r_stride = 0; a.r_f64 = 1;
    a.init_pose = d + 7 * P + 13;
    double *dout = d + nin;
    a.pose64 = dout; a.cov64 = dout + 4; a.tr64 = dout + 20; a.valid = (uint8_t *)(dout + 21);
    float *df = (float *)(dout + nout);
    a.pose = df; a.cov = df + 4; a.tr = df + 20;
    a.B = 1; a.P = P; a.z_min = clips[0]; a.istd_thres = 0.f; a.inlier_opt_only = 0;
    a.flags = MR_NO_ISTD_MASK | (result_cov ? MR_COV_CERES : MR_COV_NONE);
    a.mean_mode = MR_MEAN_SEQUENTIAL;
    int wpo = 1; while (wpo < 8 && P >= 64 * wpo * 2) wpo *= 2;
    if (launch_wpo<double>(a, wpo, sg->st) != MR_OK) return;
    double *ho = h + nin;
    if (hipMemcpyAsync(ho, dout, nout * sizeof(double), hipMemcpyDeviceToHost, sg->st) != hipSuccess ||
        hipStreamSynchronize(sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    const uint8_t ok = *(const uint8_t *)(ho + 21);
    memcpy(result_pose, ho, 4 * sizeof(double));
    *result_tr = ho[20];
    *result_val = ok ? 1 : 0;
    if (ok && result_cov) memcpy(result_cov, ho + 4, 16 * sizeof(double));
}

static int fill_decode_args(DecodeArgs &a, const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                            const float *dim_var, const float *rois, int B, int num_classes, int class_agnostic, int h, int w,
                            const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                            double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, float std_scale,
                            float ransac_thres_ratio, bool with_rois = true) {
    if (B < 0 || h < 1 || w < 1 || num_classes < 1) return MR_ERR_BAD_ARGUMENT;
    if (!all_pred || !labels || !flip || !dim || (with_rois && !rois) || !dim_means || !dim_stds || !noc_means || !noc_stds) return MR_ERR_BAD_ARGUMENT;
    memset(&a, 0, sizeof a);
    if (pred_dtype != MR_F32 && pred_dtype != MR_F16 && pred_dtype != MR_BF16) return MR_ERR_UNSUPPORTED;
    a.all_pred = all_pred; a.pred_dtype = pred_dtype; a.labels = (const long long *)labels; a.flip = flip; a.dim = dim; a.dim_var = dim_var; a.rois = rois;
    a.B = B; a.C = num_classes; a.agnostic = class_agnostic; a.h = h; a.w = w;
    a.dim_means = dim_means; a.dim_stds = dim_stds;
    a.noc_means = noc_means; a.noc_stds = noc_stds;
    // python-scalar constants of distance_invar_proj_error_coder.py:50-54, rounded the way torch rounds them
    const double e = ref_focal_y * epistemic_std_gain;
    a.k_epi = (float)(e * e);
    a.k_sd2 = (float)(proj_scaling_denominator * proj_scaling_denominator);
    const float sdf = (float)proj_scaling_denominator;
    a.sd_sq = sdf * sdf;
    a.std_scale = std_scale; a.ratio = ransac_thres_ratio; a.has_var = dim_var != nullptr;
    a.w_magic = (w > 1 && (long long)h * w < 65536) ? 0xFFFFFFFFu / (unsigned)w + 1u : 0u;
    return MR_OK;
}

int mr_noc_decode_batched(
    const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim, const float *dim_var, const float *rois,
    int B, int num_classes, int class_agnostic, int h, int w,
    const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
    double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, float std_scale, float ransac_thres_ratio,
    float *coords_2d, float *coords_2d_istd, float *coords_3d, float *dims, float *dims_var, float *ransac_thr,
    const float *coord_2d_map, int map_h, int map_w, void *stream) {
    if (B == 0) return MR_OK;
    if (coord_2d_map && (map_h < 1 || map_w < 1)) return MR_ERR_BAD_ARGUMENT;
    DecodeArgs a;
    const int rc = fill_decode_args(a, all_pred, pred_dtype, labels, flip, dim, dim_var, rois, B, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                    noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain, std_scale, ransac_thres_ratio);
    if (rc != MR_OK) return rc;
    if (!coords_2d || !coords_2d_istd || !coords_3d) return MR_ERR_BAD_ARGUMENT;
    a.c2d = coords_2d; a.istd = coords_2d_istd; a.c3d = coords_3d; a.dims = dims; a.dims_var = dims_var;
    a.thr = (ransac_thres_ratio >= 0.f) ? ransac_thr : nullptr;
    a.map2d = coord_2d_map; a.map_h = map_h; a.map_w = map_w;
    const int hw = h * w;
    const bool x4 = pred_dtype == MR_F32 && !coord_2d_map && (hw % 4 == 0) && a.w_magic != 0u &&      // w_magic: p / w by multiplication (decode_pixel_pair)
                    ((((uintptr_t)all_pred | (uintptr_t)coords_2d | (uintptr_t)coords_2d_istd | (uintptr_t)coords_3d) & 15) == 0);
    if (x4) {
        // 256 threads x one quad measured best (13.1 us per 1024 x 28x28 batch; 128 x 2 quads 14.2, 64 x 4 quads 25.5: the kernel wants threads, not trips);
        // a persistent, three-stage software-pipelined form (loads of the next quad in flight during the arithmetic; bit-identical outputs) is NOT faster:
        // 13.0 - 14.9 us against 12.5 in the same session (profiles/r04_k2_pipelined_experiment.txt)
        hipLaunchKernelGGL((noc_decode_kernel_x4<256, 1>), dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a, hw / 4);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    }
    unsigned blocks;
    if (grid_1d((long long)((hw + 255) / 256) * B, 1, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;      // (hw + 255) / 256 workgroups per object
    hipLaunchKernelGGL(noc_decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_pnp_from_head_batched(
    const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim, const float *dim_var, const float *rois,
    int B, int num_classes, int class_agnostic, int h, int w,
    const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
    double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, float std_scale, float ransac_thres_ratio,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    float z_min, float istd_thres, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag,
    float *dims, float *dims_var, const float *coord_2d_map, int map_h, int map_w,
    const float *cov_calib_logscale, float cov_corr_sd, float *cov_calib, void *stream) {
    const int P = h * w;
    if (B < 0 || P < 4 || P > 64 * kMaxChunks) return MR_ERR_BAD_ARGUMENT;
    if (coord_2d_map && (map_h < 1 || map_w < 1)) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!cam_mats || !u_range || !v_range || !valid || !pose || !tr_radius || (!cov && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    // the tile is built channel-planar, exactly the layout (and hence numpy summation order) the reference's head produces
    const int64_t s2[3] = { 2LL * P, 1, P }, s3[3] = { 3LL * P, 1, P };
    const CorrIn in{ nullptr, s2, nullptr, s2, nullptr, s3, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    PnpArgs a;
    memset(&a, 0, sizeof a);
    const int rc = fill_decode_args(a.dec, all_pred, pred_dtype, labels, flip, dim, dim_var, rois, B, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                    noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain, std_scale, ransac_thres_ratio);
    if (rc != MR_OK) return rc;
    a.dec.dims = dims; a.dec.dims_var = dims_var;
    a.dec.map2d = coord_2d_map; a.dec.map_h = map_h; a.dec.map_w = map_w;
    if (cov_calib && (!cov_calib_logscale || (flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    a.calib_logscale = cov_calib_logscale; a.corr_sd = cov_corr_sd; a.cov_calib = cov_calib;
    a.from_head = 1;
    set_inputs(a, in);
    a.B = B; a.P = P; a.z_min = (double)z_min; a.istd_thres = istd_thres; a.inlier_opt_only = inlier_opt_only; a.flags = flags;
    a.valid = valid; a.pose = pose; a.cov = cov; a.tr = tr_radius; a.mask = inlier_mask; a.diag = diag;
    a.stamps = g_stamps;
    int r;
    if ((r = choose_mean_order(a)) != MR_OK) return r;
    return launch_wpo<float>(a, lm_launch_waves(a, flags, MR_F32), (hipStream_t)stream);
}

int mr_roi_align_avg(const float *input, const float *rois, int K, int C, int H, int W, int out_h, int out_w,
                     float spatial_scale, int sampling_ratio, int aligned, float *output, void *stream) {
    if (K < 0 || C < 1 || H < 1 || W < 1 || out_h < 1 || out_w < 1) return MR_ERR_BAD_ARGUMENT;
    if (K == 0) return MR_OK;
    if (!input || !rois || !output) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d((long long)K * C * out_h * out_w, 256, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(roi_align_avg_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, input, rois, K, C, H, W, out_h, out_w,
                       spatial_scale, sampling_ratio, aligned, output);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_nms_bev_batched(const float *boxes_xyxyr, const float *scores, const int32_t *offsets, int groups, int max_group,
                       float thr, int64_t *keep, int32_t *num_keep, void *stream) {
    if (groups < 0 || max_group < 0) return MR_ERR_BAD_ARGUMENT;
    if (groups == 0) return MR_OK;
    if (!offsets || !keep || !num_keep || (max_group > 0 && (!boxes_xyxyr || !scores))) return MR_ERR_BAD_ARGUMENT;
    if (max_group > kNmsMax) return MR_ERR_UNSUPPORTED;
    int np2 = 1; while (np2 < max_group) np2 <<= 1;
    const size_t lds = (size_t)np2 * 8 + (size_t)max_group * sizeof(NmsBox) + (size_t)max_group * ((max_group + 31) / 32) * 4 + 16;
    hipLaunchKernelGGL(nms_bev_kernel, dim3(groups), dim3(256), lds, (hipStream_t)stream, boxes_xyxyr, scores, (const int *)offsets, thr,
                       (long long *)keep, (int *)num_keep);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// ---- N5: aligned rotated 3-D IoU (bbox3d_iou_calculator.py:166-192)
int mr_bbox3d_overlaps_aligned(const float *boxes, int64_t boxes_row_stride, const float *qboxes, int64_t qboxes_row_stride, int n,
                               int criterion, int z_axis, float z_center, int flags, float *iou, float *rinc, void *stream) {
    if (n < 0 || criterion < -1 || criterion > 2 || z_axis < 0 || z_axis > 2 || (flags & ~MR_IOU3D_GEOMETRIC_HEIGHT)) return MR_ERR_BAD_ARGUMENT;
    if (boxes_row_stride < 7 || qboxes_row_stride < 7) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!boxes || !qboxes || !iou) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(bbox3d_overlaps_aligned_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, boxes,
                       (long long)boxes_row_stride, qboxes, (long long)qboxes_row_stride, n, criterion, z_axis, z_center,
                       (flags & MR_IOU3D_GEOMETRIC_HEIGHT) ? 1 : 0, iou, rinc);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// ---- N6: the NOC head's training loss (uncert_projection_head.py:36-79, robust_kl_loss.py:6-30)
static int proj_check(const float *c3d, const float *pose, int64_t pose_stride, const float *K, const float *img, int n, int hw,
                      const void *out, unsigned &blocks) {
    if (n < 0 || hw < 1 || pose_stride < 4) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!c3d || !pose || !K || !img || !out) return MR_ERR_BAD_ARGUMENT;
    return grid_1d((long long)n * hw, 256, blocks) != MR_OK ? MR_ERR_UNSUPPORTED : 1;
}

int mr_uncert_projection(const float *coords_3d, const float *pose, int64_t pose_row_stride, const float *cam_intrinsic,
                         const float *img_shapes, int n, int hw, float z_min, float allowed_border, float *coords_2d, void *stream) {
    unsigned blocks;
    const int r = proj_check(coords_3d, pose, pose_row_stride, cam_intrinsic, img_shapes, n, hw, coords_2d, blocks);
    if (r != 1) return r;
    hipLaunchKernelGGL(uncert_projection_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, coords_3d, pose,
                       (long long)pose_row_stride, cam_intrinsic, img_shapes, (long long)n * hw, hw, z_min, allowed_border, coords_2d);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_uncert_projection_backward(const float *coords_3d, const float *pose, int64_t pose_row_stride, const float *cam_intrinsic,
                                  const float *img_shapes, int n, int hw, float z_min, float allowed_border, const float *grad_coords_2d,
                                  float *grad_coords_3d, void *stream) {
    unsigned blocks;
    const int r = proj_check(coords_3d, pose, pose_row_stride, cam_intrinsic, img_shapes, n, hw, grad_coords_3d, blocks);
    if (r != 1) return r;
    if (!grad_coords_2d) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(uncert_projection_backward_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, coords_3d,
                       pose, (long long)pose_row_stride, cam_intrinsic, img_shapes, (long long)n * hw, hw, z_min, allowed_border, grad_coords_2d, grad_coords_3d);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int64_t mr_robust_kl_workspace_bytes(int64_t numel) {
    if (numel <= 0) return 0;
    return ((int64_t)robust_kl_blocks(numel) * 2 * (int64_t)sizeof(double) + 255) / 256 * 256;
}

// the scalars as torch rounds them: a Python float meets an fp32 tensor as fp32; (0.5 * delta) and (1 / eps) are Python arithmetic
static KlParams kl_params(int target_mode, double delta, double eps) {
    KlParams p;
    p.identity = target_mode == -1;
    p.delta = (float)delta;
    p.half_delta = (float)(0.5 * delta);
    p.inv_max = (float)(1.0 / eps);
    return p;
}

int mr_robust_kl_loss(const float *pred, const float *logstd, int64_t numel, int target_mode, double delta, double eps, double momentum,
                      int training, int reduction, double loss_weight, float *mean_inv_std, float *loss, float *c_out, void *workspace,
                      int64_t workspace_bytes, void *stream) {
    if (numel < 1 || (target_mode != 0 && target_mode != -1) || (reduction != 0 && reduction != 1) || !(eps > 0.0)) return MR_ERR_BAD_ARGUMENT;
    if (!pred || !logstd || !mean_inv_std || !loss || !c_out || !workspace) return MR_ERR_BAD_ARGUMENT;
    if (workspace_bytes < mr_robust_kl_workspace_bytes(numel)) return MR_ERR_BAD_ARGUMENT;
    const KlParams p = kl_params(target_mode, delta, eps);
    const int blocks = robust_kl_blocks(numel);
    hipLaunchKernelGGL(robust_kl_partial_kernel, dim3(blocks), dim3(kKlThreads), 0, (hipStream_t)stream, pred, logstd, (long long)numel, p,
                       (double *)workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(robust_kl_fold_kernel, dim3(1), dim3(kKlThreads), 0, (hipStream_t)stream, (const double *)workspace, blocks,
                       (long long)numel, training ? 1 : 0, (float)(1.0 - momentum), (float)momentum, reduction == 0 ? 1 : 0, (float)loss_weight,
                       mean_inv_std, loss, c_out);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_robust_kl_loss_backward(const float *pred, const float *logstd, int64_t numel, int target_mode, double delta, double eps,
                               int reduction, double loss_weight, const float *grad_loss, const float *c, float *grad_pred,
                               float *grad_logstd, void *stream) {
    if (numel < 1 || (target_mode != 0 && target_mode != -1) || (reduction != 0 && reduction != 1) || !(eps > 0.0)) return MR_ERR_BAD_ARGUMENT;
    if (!pred || !logstd || !grad_loss || !c || !grad_pred || !grad_logstd) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d(numel, kKlThreads, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(robust_kl_backward_kernel, dim3(blocks), dim3(kKlThreads), 0,
                       (hipStream_t)stream, pred, logstd, (long long)numel, kl_params(target_mode, delta, eps), grad_loss, c,
                       (float)loss_weight, reduction == 0 ? 1 : 0, grad_pred, grad_logstd);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// ---- N2: KITTI evaluator (eval.py / rotate_iou.py of core/evaluation/kitti_utils)
int mr_kitti_overlaps(int metric, int arith32, int out32, int n_img, const int64_t *dt_off, const int64_t *gt_off, const int64_t *ov_off,
                      int64_t total_pairs, const double *dt_box, const double *gt_box, double *overlaps, void *stream) {
    if (metric < 0 || metric > 2 || n_img < 0 || total_pairs < 0) return MR_ERR_BAD_ARGUMENT;
    if (n_img == 0 || total_pairs == 0) return MR_OK;
    if (!dt_off || !gt_off || !ov_off || !dt_box || !gt_box || !overlaps) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d(total_pairs, 256, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kitti_overlap_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, metric, arith32, out32, n_img,
                       (const long long *)dt_off, (const long long *)gt_off, (const long long *)ov_off, dt_box, gt_box, overlaps);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int64_t mr_kitti_match_workspace_bytes(int n_img, int n_combo) {
    if (n_img < 0 || n_combo < 0) return 0;
    return (int64_t)n_combo * kEvalSamples * (int64_t)n_img * (3 * sizeof(int) + sizeof(double)) + 64;
}

int mr_kitti_match(int second_pass, int metric, int compute_aos, int alpha32, int dtdata32, int n_img, int max_det,
                   const int64_t *dt_off, const int64_t *gt_off, const int64_t *ov_off, const int64_t *dc_off,
                   int64_t total_dt, int64_t total_gt,
                   const double *overlaps, const double *dt_box, const double *dt_alpha, const double *gt_alpha, const double *dc_box,
                   const int8_t *ign_gt, const int8_t *ign_dt, int n_combo, const int32_t *combo_cd, const double *combo_min_overlap,
                   const double *thresholds, const int32_t *n_thr, double *match_score, double *pr,
                   void *workspace, int64_t workspace_bytes, void *stream) {
    if (n_img < 0 || n_combo < 0 || metric < 0 || metric > 2) return MR_ERR_BAD_ARGUMENT;
    if (n_img == 0 || n_combo == 0) return MR_OK;
    if (max_det > kEvalMaxDet) return MR_ERR_UNSUPPORTED;
    if (!dt_off || !gt_off || !ov_off || !dc_off || !ign_gt || !ign_dt || !combo_cd || !combo_min_overlap) return MR_ERR_BAD_ARGUMENT;
    MatchArgs a;
    a.second_pass = second_pass; a.metric = metric; a.compute_aos = compute_aos; a.alpha32 = alpha32; a.dtdata32 = dtdata32;
    a.n_img = n_img; a.n_combo = n_combo; a.total_gt = total_gt; a.total_dt = total_dt;
    a.dt_off = (const long long *)dt_off; a.gt_off = (const long long *)gt_off; a.ov_off = (const long long *)ov_off; a.dc_off = (const long long *)dc_off;
    a.ov = overlaps; a.dt_box = dt_box; a.dt_alpha = dt_alpha; a.gt_alpha = gt_alpha; a.dc_box = dc_box;
    a.ign_gt = (const signed char *)ign_gt; a.ign_dt = (const signed char *)ign_dt;
    a.combo_cd = (const int *)combo_cd; a.combo_min_overlap = combo_min_overlap;
    a.thresholds = thresholds; a.n_thr = (const int *)n_thr; a.match_score = match_score;
    a.st_tp = a.st_fp = a.st_fn = nullptr; a.st_sim = nullptr;
    long long threads = (long long)n_combo * n_img;
    if (second_pass) {
        if (!thresholds || !n_thr || !pr || !workspace || workspace_bytes < mr_kitti_match_workspace_bytes(n_img, n_combo)) return MR_ERR_BAD_ARGUMENT;
        const long long cells = (long long)n_combo * kEvalSamples * n_img;
        a.st_sim = (double *)workspace;                       // doubles first (alignment), then the three int planes
        a.st_tp = (int *)(a.st_sim + cells); a.st_fp = a.st_tp + cells; a.st_fn = a.st_fp + cells;
        threads *= kEvalSamples;
    } else if (!match_score) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d(threads, 128, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kitti_match_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    if (second_pass) {
        hipLaunchKernelGGL(kitti_reduce_kernel, dim3((n_combo * kEvalSamples + 63) / 64), dim3(64), 0, (hipStream_t)stream, n_img, n_combo,
                           (const int *)n_thr, a.st_tp, a.st_fp, a.st_fn, a.st_sim, pr);
        HIP_TRY(hipGetLastError());
    }
    return MR_OK;
}

// The 7-parameter entry points of the reference's C ABI (ext.h:15-43).  Host fp64 buffers; one object; blocking.
static void noc_host(int full_cov, double *pts2d, double *pts3d, double *wgt2d, double *logdim, double *logdim_wgt, double *K,
                     double *init_dimpose, int *result_val, double *result_dimpose, int pn, double *clips, double delta) {
    *result_val = 0;
    memcpy(result_dimpose, init_dimpose, 7 * sizeof(double));            // pnp_uncert_cpu.cpp:309,351
    if (pn < 0) return;
    const int ws = full_cov ? 3 : 2;
    // staging, in doubles: [pts2d 2n | pts3d 3n | wgt ws*n | logdim 3 | logdim_wgt 3 | K 9 | init 7 | clips 5 || out 7 | val (int, 8 bytes)]
    const size_t n = (size_t)pn;
    const size_t nin = (2 + 3 + ws) * n + 3 + 3 + 9 + 7 + 5, nout = 7 + 1;
    HostStage *sg = stage_acquire((nin + nout) * sizeof(double));
    if (!sg) return;
    std::lock_guard<std::mutex> lk(sg->mu, std::adopt_lock);
    double *h = (double *)sg->hbuf, *d = (double *)sg->dbuf;
    double *q = h;
    memcpy(q, pts2d, sizeof(double) * 2 * n); q += 2 * n;
    memcpy(q, pts3d, sizeof(double) * 3 * n); q += 3 * n;
    memcpy(q, wgt2d, sizeof(double) * ws * n); q += ws * n;
    memcpy(q, logdim, sizeof(double) * 3); q += 3;
    memcpy(q, logdim_wgt, sizeof(double) * 3); q += 3;
    memcpy(q, K, sizeof(double) * 9); q += 9;
    memcpy(q, init_dimpose, sizeof(double) * 7); q += 7;
    memcpy(q, clips, sizeof(double) * 5);
    if (hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    NocArgs a;
    memset(&a, 0, sizeof a);
    a.pts2d = d; a.pts3d = d + 2 * n; a.wgt2d = d + 5 * n; a.logdim = d + (5 + ws) * n; a.logdim_wgt = a.logdim + 3; a.K = a.logdim + 6;
    a.init = a.logdim + 15; a.clips = a.logdim + 22; a.out_dimpose = d + nin; a.out_val = (int *)(d + nin + 7); a.out_diag = nullptr;
    a.K_batch = 1; a.clips_batch = 1; a.B = 1;
    a.delta = delta; a.pn = pn; a.full_cov = full_cov;
    hipLaunchKernelGGL(pnp_noc_kernel, dim3(1), dim3(256), kNocLds, sg->st, a);
    if (hipGetLastError() != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    double *ho = h + nin;
    if (hipMemcpyAsync(ho, d + nin, nout * sizeof(double), hipMemcpyDeviceToHost, sg->st) != hipSuccess ||
        hipStreamSynchronize(sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    memcpy(result_dimpose, ho, 7 * sizeof(double));
    *result_val = *(const int *)(ho + 7);
}

void pnp_noc_uncert(double *pts2d, double *pts3d, double *wgt2d, double *logdim, double *logdim_wgt, double *K,
                    double *init_dimpose, int *result_val, double *result_dimpose, int pn, double *clips, double delta) {
    noc_host(0, pts2d, pts3d, wgt2d, logdim, logdim_wgt, K, init_dimpose, result_val, result_dimpose, pn, clips, delta);
}

void pnp_noc_cov_uncert(double *pts2d, double *pts3d, double *wgt2d, double *logdim, double *logdim_wgt, double *K,
                        double *init_dimpose, int *result_val, double *result_dimpose, int pn, double *clips, double delta) {
    noc_host(1, pts2d, pts3d, wgt2d, logdim, logdim_wgt, K, init_dimpose, result_val, result_dimpose, pn, clips, delta);
}

// Batched form of the two 7-parameter solvers (device fp64 buffers, one workgroup per object; pnp_noc_kernel.inc)
int mr_pnp_noc_batched(int full_cov, const double *pts2d, const double *pts3d, const double *wgt2d, const double *logdim, const double *logdim_wgt,
                       const double *K, int K_batch, const double *init_dimpose, const double *clips, int clips_batch, double delta, int B, int pn,
                       double *result_dimpose, int32_t *result_val, double *diag, void *stream) {
    if (B < 0 || pn < 0 || (K_batch != 1 && K_batch != B) || (clips_batch != 1 && clips_batch != B)) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if ((pn > 0 && (!pts2d || !pts3d || !wgt2d)) || !logdim || !logdim_wgt || !K || !init_dimpose || !clips || !result_dimpose || !result_val) return MR_ERR_BAD_ARGUMENT;
    NocArgs a;
    memset(&a, 0, sizeof a);
    a.pts2d = pts2d; a.pts3d = pts3d; a.wgt2d = wgt2d; a.logdim = logdim; a.logdim_wgt = logdim_wgt; a.K = K; a.init = init_dimpose; a.clips = clips;
    a.K_batch = K_batch; a.clips_batch = clips_batch; a.delta = delta; a.pn = pn; a.full_cov = full_cov ? 1 : 0; a.B = B;
    a.out_dimpose = result_dimpose; a.out_val = (int *)result_val; a.out_diag = diag;
    hipLaunchKernelGGL(pnp_noc_kernel, dim3(B), dim3(256), kNocLds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// ---- N7: the score head's eval-mode forward with its epilogue (mlp_score_head.py:94-115, monorun_roi_head.py:544-550); include/monorun_heads.h
int mr_score_head_forward(const float *reg_fc_out, int64_t reg_fc_out_row_stride, const float *yaw, int64_t yaw_row_stride,
                          const float *t_vec, int64_t t_vec_row_stride, const float *pose_cov, const float *dimensions,
                          int64_t dimensions_row_stride, const uint8_t *ret_val, const float *scores_2d, const float *params,
                          int64_t params_numel, int n, int c1, int c2, int flags, float *scores, void *stream) {
    if (n < 0 || c1 < 1 || c1 > MR_SCORE_MAX_C1 || c2 < 1 || c2 > MR_SCORE_MAX_C2 || (flags & ~MR_SCORE_SIGMOID)) return MR_ERR_BAD_ARGUMENT;
    if (reg_fc_out_row_stride < c1 || yaw_row_stride < 1 || t_vec_row_stride < 3 || dimensions_row_stride < 3) return MR_ERR_BAD_ARGUMENT;
    if (params_numel != score_layout(c1, c2).numel || ((uintptr_t)params & 15)) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!reg_fc_out || !yaw || !t_vec || !pose_cov || !dimensions || !params || !scores) return MR_ERR_BAD_ARGUMENT;
    ScoreArgs a;
    a.reg = reg_fc_out; a.yaw = yaw; a.t = t_vec; a.cov = pose_cov; a.dim = dimensions;
    a.reg_stride = reg_fc_out_row_stride; a.yaw_stride = yaw_row_stride; a.t_stride = t_vec_row_stride; a.dim_stride = dimensions_row_stride;
    a.ret_val = ret_val; a.scores_2d = scores_2d; a.params = params; a.n = n; a.c1 = c1; a.c2 = c2;
    a.sigmoid = (flags & MR_SCORE_SIGMOID) ? 1 : 0; a.out = scores;
    hipLaunchKernelGGL(score_head_forward_kernel, dim3((unsigned)(((long long)n + kScoreRows - 1) / kScoreRows)), dim3(kScoreThreads), 0,
                       (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// ---- N9: the global head's Monte-Carlo eval forward, factored over the channel mask (fc_extractor_monte_carlo.py:41-63); include/monorun_global.h
static int global_head_check(int n, int C, int A, int F, int J, int S) {
    if (n < 0 || C < 1 || A < 1 || F < 1 || J < 1 || S < 2) return MR_ERR_BAD_ARGUMENT;
    if (C > MR_GLOBAL_MAX_CHANNELS || A > MR_GLOBAL_MAX_CHANNELS || F > MR_GLOBAL_MAX_CHANNELS || J > MR_GLOBAL_MAX_OUT || S > MR_GLOBAL_MAX_SAMPLES)
        return MR_ERR_UNSUPPORTED;
    const long long lim = 0x7fffffffLL, sn = (long long)S * n, ca = (long long)C * A;
    if (n * ca > lim || F * ca > lim || sn * F > lim || sn * C > lim || sn * J > lim) return MR_ERR_UNSUPPORTED;
    return MR_OK;
}

static size_t global_head_pass_floats(int nc, int C, int F, int J, int S) {
    return (size_t)nc * ((size_t)C * F + 2 * (size_t)S * F + (size_t)S * J);
}

size_t mr_global_head_mc_workspace_bytes(int n, int in_channels, int area, int fc_channels, int out_channels, int num_samples) {
    if (global_head_check(n, in_channels, area, fc_channels, out_channels, num_samples) != MR_OK) return 0;
    return sizeof(float) * global_head_pass_floats(n < kGhChunk ? n : kGhChunk, in_channels, fc_channels, out_channels, num_samples);
}

int mr_global_head_mc_forward(const float *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *w_reg,
                              const float *b_reg, const uint8_t *keep0, const uint8_t *keep1, const uint8_t *keep2, float q0, float q1,
                              int n, int in_channels, int area, int fc_channels, int out_channels, int num_samples, void *workspace,
                              size_t workspace_bytes, float *mean, float *var, float *reg_fc_out, float *samples, void *stream) {
    static_assert(kGhChunk == MR_GLOBAL_CHUNK, "the header states the pass size");
    const int C = in_channels, A = area, F = fc_channels, J = out_channels, S = num_samples;
    const int rc = global_head_check(n, C, A, F, J, S);
    if (rc != MR_OK) return rc;
    if (n == 0) return MR_OK;
    if (!x || !w1 || !b1 || !w2 || !b2 || !w_reg || !b_reg || !keep0 || !keep1 || !keep2 || !workspace || !mean || !var || !reg_fc_out)
        return MR_ERR_BAD_ARGUMENT;
    const int chunk = n < kGhChunk ? n : kGhChunk;
    if (((uintptr_t)workspace & 3) || workspace_bytes < sizeof(float) * global_head_pass_floats(chunk, C, F, J, S)) return MR_ERR_BAD_ARGUMENT;
    GhArgs a;
    a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.wr = w_reg; a.br = b_reg;
    a.keep0 = keep0; a.keep1 = keep1; a.keep2 = keep2; a.q0 = q0; a.q1 = q1;
    a.n = n; a.C = C; a.A = A; a.F = F; a.J = J; a.S = S;
    a.P = (float *)workspace;
    a.h1 = a.P + (size_t)chunk * C * F;
    a.h2 = a.h1 + (size_t)chunk * S * F;
    a.ys = a.h2 + (size_t)chunk * S * F;
    a.mean = mean; a.var = var; a.reg = reg_fc_out; a.samples = samples;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nt = (unsigned)((F + kGhBN - 1) / kGhBN);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        a.i0 = i0; a.nc = n - i0 < chunk ? n - i0 : chunk;
        const unsigned rows = (unsigned)(S * a.nc);
        hipLaunchKernelGGL(gh_p_kernel, dim3(nt, (unsigned)((a.nc + kGhBM - 1) / kGhBM), (unsigned)C), dim3(kGhThreads), 0, st, a);
        hipLaunchKernelGGL(gh_h1_kernel, dim3(nt, (unsigned)((S + kGhBM - 1) / kGhBM), (unsigned)a.nc), dim3(kGhThreads), 0, st, a);
        hipLaunchKernelGGL(gh_h2_kernel, dim3(nt, (rows + kGhBM - 1) / kGhBM, 1), dim3(kGhThreads), 0, st, a);
        hipLaunchKernelGGL(gh_out_kernel, dim3((rows + kGhOutRows - 1) / kGhOutRows), dim3(64 * kGhOutRows), 0, st, a);
        hipLaunchKernelGGL(gh_stats_kernel, dim3((unsigned)a.nc), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return MR_OK;
}

// ---- N8: the NOC head's training decode, forward and backward (monorun_roi_head.py:189-217, :374-394); include/monorun_train.h
static int fill_decode_train_args(DecodeTrainArgs &t, const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                                  const float *dim_var, int n, int num_classes, int class_agnostic, int h, int w,
                                  const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                                  double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain) {
    memset(&t, 0, sizeof t);
    const int rc = fill_decode_args(t.d, all_pred, pred_dtype, labels, flip, dim, dim_var, nullptr, n, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                    noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain, 1.0f, -1.0f, false);
    if (rc != MR_OK) return rc;
    if ((long long)h * w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    t.sdf = (float)proj_scaling_denominator;
    return MR_OK;
}

int mr_noc_decode_train(const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                        const float *dim_var, const float *distances, int n, int num_classes, int class_agnostic, int h, int w,
                        const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                        double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain, double distance_min,
                        float *noc_pred, float *proj_logstd, float *coords_3d, float *coords_3d_var, float *proj_logstd_px,
                        float *dims, float *dims_var, void *stream) {
    if (n == 0) return MR_OK;
    DecodeTrainArgs t;
    const int rc = fill_decode_train_args(t, all_pred, pred_dtype, labels, flip, dim, dim_var, n, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                          noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain);
    if (rc != MR_OK) return rc;
    if (!noc_pred || !proj_logstd || !coords_3d || !proj_logstd_px || !dims || (dim_var && (!coords_3d_var || !dims_var))) return MR_ERR_BAD_ARGUMENT;
    t.distances = distances; t.dist_min = (float)distance_min;
    t.noc = noc_pred; t.ls = proj_logstd; t.d.c3d = coords_3d; t.c3d_var = coords_3d_var; t.lspx = proj_logstd_px; t.d.dims = dims; t.d.dims_var = dims_var;
    return launch_noc_decode_train(t, (hipStream_t)stream);
}

int mr_noc_decode_train_backward(const void *all_pred, int pred_dtype, const int64_t *labels, const uint8_t *flip, const float *dim,
                                 const float *dim_var, int n, int num_classes, int class_agnostic, int h, int w,
                                 const float *dim_means, const float *dim_stds, const float *noc_means, const float *noc_stds,
                                 double proj_scaling_denominator, double ref_focal_y, double epistemic_std_gain,
                                 const float *grad_noc_pred, const float *grad_proj_logstd, const float *grad_coords_3d,
                                 const float *grad_coords_3d_var, const float *grad_proj_logstd_px, const float *grad_dims,
                                 const float *grad_dims_var, void *grad_all_pred, float *grad_dim, float *grad_dim_var, void *stream) {
    if (n == 0) return MR_OK;
    DecodeTrainArgs t;
    const int rc = fill_decode_train_args(t, all_pred, pred_dtype, labels, flip, dim, dim_var, n, num_classes, class_agnostic, h, w, dim_means, dim_stds,
                                          noc_means, noc_stds, proj_scaling_denominator, ref_focal_y, epistemic_std_gain);
    if (rc != MR_OK) return rc;
    if (!grad_all_pred || !grad_dim || (dim_var && !grad_dim_var)) return MR_ERR_BAD_ARGUMENT;
    t.g_noc = grad_noc_pred; t.g_ls = grad_proj_logstd; t.g_c3d = grad_coords_3d; t.g_c3d_var = grad_coords_3d_var; t.g_lspx = grad_proj_logstd_px;
    t.g_dims = grad_dims; t.g_dims_var = grad_dims_var;
    t.grad_all_pred = grad_all_pred; t.grad_dim = grad_dim; t.grad_dim_var = grad_dim_var;
    return launch_noc_decode_train_backward(t, (hipStream_t)stream);
}

// ---- N10: the NOC head trunk's upsampler, CARAFEPack's normaliser + reassembly fused (mmcv.ops.carafe); include/monorun_carafe.h
static int carafe_fill(CarafeArgs &a, int n, int C, int h, int w, int k, int G, int s) {
    static_assert(kCarafeTile == MR_CARAFE_TILE && kCarafeChunk == MR_CARAFE_CHUNK, "the header states the tiling");
    if (n < 0 || C < 1 || h < 1 || w < 1 || G < 1 || C % G != 0) return MR_ERR_BAD_ARGUMENT;
    if (!(k == 1 || k == 3 || k == 5 || k == 7) || !(s == 1 || s == 2 || s == 4)) return MR_ERR_UNSUPPORTED;
    // offsets inside one RoI are 32-bit in the kernels: its channels x output pixels and its logits must fit
    if ((long long)C * h * s * w * s > 0x7fffffffLL || (long long)G * k * k * s * s * h * w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    memset(&a, 0, sizeof a);
    a.N = n; a.C = C; a.H = h; a.W = w; a.G = G; a.s = s; a.ls = s == 4 ? 2 : s == 2 ? 1 : 0;
    a.Cg = C / G; a.cpg = (a.Cg + kCarafeChunk - 1) / kCarafeChunk;
    a.tiles_x = (w + kCarafeTile - 1) / kCarafeTile; a.tiles_y = (h + kCarafeTile - 1) / kCarafeTile;
    return MR_OK;
}

// one of the three kernels at the up_kernel the arguments name: `which` 0 forward, 1 backward masks / grad_m, 2 backward grad_x
#define MR_CARAFE_LAUNCH(K) do { \
        if (which == 0) hipLaunchKernelGGL(carafe_pack_forward_kernel<K>, dim3(nb), dim3(kCarafeThreads), 0, st, a); \
        else if (which == 1) hipLaunchKernelGGL(carafe_pack_backward_mask_kernel<K>, dim3(nb), dim3(kCarafeThreads), 0, st, a); \
        else hipLaunchKernelGGL(carafe_pack_backward_input_kernel<K>, dim3(nb), dim3(kCarafeThreads), 0, st, a); \
    } while (0)
static int carafe_launch(int which, int k, long long blocks, hipStream_t st, const CarafeArgs &a) {
    unsigned nb;
    if (grid_1d(blocks, 1, nb) != MR_OK) return MR_ERR_UNSUPPORTED;
    switch (k) {
        case 1: MR_CARAFE_LAUNCH(1); break;
        case 3: MR_CARAFE_LAUNCH(3); break;
        case 5: MR_CARAFE_LAUNCH(5); break;
        default: MR_CARAFE_LAUNCH(7); break;
    }
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
#undef MR_CARAFE_LAUNCH

int mr_carafe_pack_forward(const float *x, const float *m, int n, int channels, int h, int w, int up_kernel, int up_group, int scale_factor,
                           float *out, void *stream) {
    CarafeArgs a;
    const int rc = carafe_fill(a, n, channels, h, w, up_kernel, up_group, scale_factor);
    if (rc != MR_OK) return rc;
    if (n == 0) return MR_OK;
    if (!x || !m || !out) return MR_ERR_BAD_ARGUMENT;
    a.x = x; a.m = m; a.out = out;
    return carafe_launch(0, up_kernel, (long long)n * a.G * a.cpg * a.tiles_x * a.tiles_y, (hipStream_t)stream, a);
}

size_t mr_carafe_backward_workspace_bytes(int n, int channels, int h, int w, int up_kernel, int up_group, int scale_factor) {
    CarafeArgs a;
    if (carafe_fill(a, n, channels, h, w, up_kernel, up_group, scale_factor) != MR_OK) return 0;
    return sizeof(float) * (size_t)n * up_group * up_kernel * up_kernel * ((size_t)h * scale_factor) * ((size_t)w * scale_factor);
}

int mr_carafe_pack_backward(const float *x, const float *m, const float *grad_out, int n, int channels, int h, int w, int up_kernel,
                            int up_group, int scale_factor, void *workspace, size_t workspace_bytes, float *grad_x, float *grad_m,
                            void *stream) {
    CarafeArgs a;
    const int rc = carafe_fill(a, n, channels, h, w, up_kernel, up_group, scale_factor);
    if (rc != MR_OK) return rc;
    if (n == 0 || (!grad_x && !grad_m)) return MR_OK;
    if (!x || !m || !grad_out) return MR_ERR_BAD_ARGUMENT;
    if (grad_x && (!workspace || ((uintptr_t)workspace & 3) ||
                   workspace_bytes < mr_carafe_backward_workspace_bytes(n, channels, h, w, up_kernel, up_group, scale_factor)))
        return MR_ERR_BAD_ARGUMENT;
    a.x = x; a.m = m; a.go = grad_out; a.gx = grad_x; a.gm = grad_m; a.wn = grad_x ? (float *)workspace : nullptr;
    const long long tiles = (long long)a.tiles_x * a.tiles_y;
    const int r1 = carafe_launch(1, up_kernel, (long long)n * a.G * tiles * scale_factor * scale_factor, (hipStream_t)stream, a);
    if (r1 != MR_OK || !grad_x) return r1;
    return carafe_launch(2, up_kernel, (long long)n * a.G * a.cpg * tiles, (hipStream_t)stream, a);
}

// ---- N9: the NOC head's LiDAR supervision (monorun_targets.h; masked_dense_target.py, noc_coder.py:17-48, smooth_l1_loss.py)
int mr_noc_dense_target(int num_images, const float *const *coords_3d, const float *const *coords_3d_mask, const float *const *dimensions,
                        const int64_t *dimensions_row_stride, const int32_t *map_h, const int32_t *map_w, const int32_t *num_gt,
                        const uint8_t *flip, const float *rois, const int32_t *roi_img, const int64_t *roi_gt, int n, int h, int w,
                        const float *target_means, const float *target_stds, double eps_coder, double eps_target,
                        float *targets, float *weights, int32_t *counts, void *stream) {
    if (n < 0 || num_images < 0 || h < 1 || w < 1) return MR_ERR_BAD_ARGUMENT;
    if (n == 0) return MR_OK;
    if (!rois || !roi_img || !roi_gt || !target_means || !target_stds || !targets || !weights || !counts) return MR_ERR_BAD_ARGUMENT;
    if (num_images > 0 && (!coords_3d || !coords_3d_mask || !dimensions || !dimensions_row_stride || !map_h || !map_w || !num_gt || !flip))
        return MR_ERR_BAD_ARGUMENT;
    if (num_images > kNocMaxImages || (long long)n * h * w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    NocTargetArgs a;
    memset(&a, 0, sizeof a);
    for (int j = 0; j < num_images; ++j) {
        if (map_h[j] < 1 || map_w[j] < 1 || num_gt[j] < 0) return MR_ERR_BAD_ARGUMENT;
        if (num_gt[j] > 0 && (!coords_3d[j] || !coords_3d_mask[j] || !dimensions[j] || dimensions_row_stride[j] < 3)) return MR_ERR_BAD_ARGUMENT;
        NocImage &im = a.img[j];
        im.coords = coords_3d[j]; im.mask = coords_3d_mask[j]; im.dims = dimensions[j]; im.dims_stride = (long long)dimensions_row_stride[j];
        im.H = map_h[j]; im.W = map_w[j]; im.G = num_gt[j]; im.flip = flip[j] ? 1 : 0;
    }
    a.num_images = num_images;
    a.rois = rois; a.roi_img = (const int *)roi_img; a.roi_gt = (const long long *)roi_gt;
    a.n = n; a.h = h; a.w = w;
    a.means = target_means; a.stds = target_stds;
    a.eps_c = (float)eps_coder; a.eps_t = (float)eps_target;          // a Python float meets an fp32 tensor as fp32
    a.targets = targets; a.weights = weights; a.counts = (int *)counts;
    hipLaunchKernelGGL(noc_dense_target_kernel, dim3((unsigned)n), dim3(kNocThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(noc_target_normalise_kernel, dim3((unsigned)n), dim3(kNocThreads), 0, (hipStream_t)stream, (const int *)counts, n, h * w,
                       a.eps_t, weights);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int64_t mr_smooth_l1_mod_workspace_bytes(int64_t numel) {
    if (numel <= 0) return 0;
    return ((int64_t)robust_kl_blocks(numel) * (int64_t)sizeof(double) + 255) / 256 * 256;
}

static int sl1_params(const void *pred, const void *target, const void *weight, int weight_mode, int64_t numel, int channels, int64_t hw,
                      double beta, int reduction, Sl1Params &p) {
    if (numel < 1 || !(beta > 0.0) || (reduction != 0 && reduction != 1) || weight_mode < 0 || weight_mode > 2) return MR_ERR_BAD_ARGUMENT;
    if (!pred || !target || (weight_mode != 0 && !weight)) return MR_ERR_BAD_ARGUMENT;
    p.beta = (float)beta; p.half_beta = (float)(0.5 * beta); p.weight_mode = weight_mode; p.chw = 1; p.hw = 1;
    if (weight_mode == 2) {
        if (channels < 1 || hw < 1 || numel % ((int64_t)channels * hw) != 0) return MR_ERR_BAD_ARGUMENT;
        p.chw = (long long)channels * hw; p.hw = (long long)hw;
    }
    return MR_OK;
}

int mr_smooth_l1_mod_loss(const float *pred, const float *target, const float *weight, int weight_mode, int64_t numel, int channels, int64_t hw,
                          double beta, int reduction, double loss_weight, float *loss, void *workspace, int64_t workspace_bytes, void *stream) {
    Sl1Params p;
    const int r = sl1_params(pred, target, weight, weight_mode, numel, channels, hw, beta, reduction, p);
    if (r != MR_OK) return r;
    if (!loss || !workspace || workspace_bytes < mr_smooth_l1_mod_workspace_bytes(numel)) return MR_ERR_BAD_ARGUMENT;
    const int blocks = robust_kl_blocks(numel);
    hipLaunchKernelGGL(smooth_l1_mod_loss_kernel, dim3(blocks), dim3(kKlThreads), 0, (hipStream_t)stream, pred, target, weight, (long long)numel, p,
                       (double *)workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(smooth_l1_mod_finish_kernel, dim3(1), dim3(kKlThreads), 0, (hipStream_t)stream, (const double *)workspace, blocks,
                       (long long)numel, reduction == 0 ? 1 : 0, (float)loss_weight, loss);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_smooth_l1_mod_loss_backward(const float *pred, const float *target, const float *weight, int weight_mode, int64_t numel, int channels,
                                   int64_t hw, double beta, int reduction, double loss_weight, const float *grad_loss, float *grad_pred,
                                   void *stream) {
    Sl1Params p;
    const int r = sl1_params(pred, target, weight, weight_mode, numel, channels, hw, beta, reduction, p);
    if (r != MR_OK) return r;
    if (!grad_loss || !grad_pred) return MR_ERR_BAD_ARGUMENT;
    unsigned blocks;
    if (grid_1d(numel, kKlThreads, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(smooth_l1_mod_loss_backward_kernel, dim3(blocks), dim3(kKlThreads), 0, (hipStream_t)stream, pred, target, weight,
                       (long long)numel, p, grad_loss, (float)loss_weight, reduction == 0 ? 1 : 0, grad_pred);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// development aid (not in the public header): device buffer of (B,10) u64 cycle stamps, or NULL to disable
void mr_pnp_debug_set_stamps(unsigned long long *dev_ptr) { g_stamps = dev_ptr; }
#ifdef MR_DEBUG_STAMPS
// -DMR_DEBUG_STAMPS builds only: device buffer of (B,24) u64 stamps of the consensus launches (EPC_STAMP, tools/gpu_consensus_stamps.py), or NULL
void mr_pnp_debug_set_consensus_stamps(unsigned long long *dev_ptr) { g_cons_stamps = dev_ptr; }
#endif

// development aids for the tests (not in the public header):
// waves per object of the LM / covariance launch over `objects` objects x P points of `in_dtype` with `flags` (MR_WAVES bits honoured),
// after the default flow's initialiser when `after_init` is set (mr_pnp_uncert_from_init_* / _from_epnp_grouped), else the fast mode's
int mr_debug_launch_waves(int objects, int P, int in_dtype, int flags, int after_init) {
    if (objects < 1 || P < 4 || P > 64 * kMaxChunks || (in_dtype != MR_F32 && in_dtype != MR_F16 && in_dtype != MR_F64)) return MR_ERR_BAD_ARGUMENT;
    static const uint8_t any_mask = 0;
    PnpArgs a;
    memset(&a, 0, sizeof a);
    a.B = objects; a.P = P; a.flags = flags;
    a.init_mask = after_init ? &any_mask : nullptr;
    return lm_launch_waves(a, flags, in_dtype);
}

// block_sum_packed<wpo, 10> on `partials` (device, 64 wpo x 10 doubles, lane-major) -> `out` (device, wpo x 10: every wave's totals)
int mr_debug_block_sum(int wpo, const double *partials, double *out, void *stream) {
    if (!partials || !out) return MR_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    switch (wpo) {
        case 1: hipLaunchKernelGGL(block_sum_probe_kernel<1>, dim3(1), dim3(64), 0, st, partials, out); break;
        case 2: hipLaunchKernelGGL(block_sum_probe_kernel<2>, dim3(1), dim3(128), 0, st, partials, out); break;
        case 3: hipLaunchKernelGGL(block_sum_probe_kernel<3>, dim3(1), dim3(192), 0, st, partials, out); break;
        case 4: hipLaunchKernelGGL(block_sum_probe_kernel<4>, dim3(1), dim3(256), 0, st, partials, out); break;
        case 8: hipLaunchKernelGGL(block_sum_probe_kernel<8>, dim3(1), dim3(512), 0, st, partials, out); break;
        default: return MR_ERR_BAD_ARGUMENT;
    }
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

}  // extern "C"
