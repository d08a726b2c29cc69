// projection_loss_kernel.inc — N6 (DESIGN.md §12): the NOC head's training loss, the reference's UncertProjectionHead.forward
// (monorun/models/roi_heads/bbox_3d_heads/reprojection_heads/uncert_projection_head.py:36-79) and its RobustKLLoss
// (monorun/models/losses/robust_kl_loss.py:6-30), forward and backward.  The head's encode of (proj - roi) between the two stays
// in torch (proj_error_coder.encode, distance_invar_proj_error_coder.py:20-31).
//
// Projection: one thread per RoI pixel, both image channels per thread (the backward sums both into X, Y and Z).  Pose rows may
// have any row stride (the training caller passes the slice pos_bboxes_3d[:, 3:7]).
//   R_y(yaw) with sin / cos computed in fp64 and rounded to fp32; P_R = K @ R and P_t = K @ t in fp32; proj = P_R @ X + P_t;
//   every three-term dot product summed left to right, contraction off; uv = proj[:2] / clamp(z, min=z_min) (IEEE division);
//   uv = min(clamp(uv, min=-border), [W, H] + border).  Clamps and min propagate NaN as torch's do (no fminf / fmaxf).
//   Backward, torch's rules at ties: a clamp passes the gradient at its bound; torch.min gives half to each side of a tie.
// Robust KL loss: per element
//   diff = |pred| (target 0) or pred (target -1);  inv = min(mr_expf(-logstd), fp32(1/eps));  dw = diff * inv;
//   raw = (dw < delta ? 0.5 * dw^2 : delta * (dw - 0.5 * delta)) + logstd
//   Launch 1 (partials): a grid that depends on numel only; each workgroup writes fp64 sums of inv and raw to the workspace.
//   Launch 2 (fold): one workgroup adds the partials in a fixed order, updates mean_inv_std in place in training mode
//   (m = m * fp32(1 - momentum); m = m + fp32(momentum) * fp32(sum_inv / numel)), takes c = clamp(m, min=1e-6) and writes
//   loss = fp32(loss_weight) * fp32(sum_raw / c [/ numel]) and c.  No floating-point atomics: bitwise reproducible.
//   Backward (one launch): reads c and the upstream gradient from device memory, never the buffer.
// No scratch; 256-thread workgroups; results are ordinary vector stores.

constexpr int kKlThreads = 256;
constexpr int kKlItems = 8;                 // elements per thread before the grid stops growing
constexpr int kKlMaxBlocks = 1024;

__host__ __device__ inline int robust_kl_blocks(long long numel) {
    long long b = (numel + (long long)kKlThreads * kKlItems - 1) / ((long long)kKlThreads * kKlItems);
    return (int)(b < 1 ? 1 : (b > kKlMaxBlocks ? kKlMaxBlocks : b));
}

struct ProjSetup { float pr[9], pt[3], umax, vmax; };

// Per-object P_R = K @ R_y(yaw), P_t = K @ t and the upper clamp bounds [W, H] + border.
__device__ __forceinline__ ProjSetup proj_setup(const float *__restrict__ pose, long long pose_stride, const float *__restrict__ K,
                                                const float *__restrict__ img, long long o, float border) {
#pragma clang fp contract(off)
    ProjSetup s;
    const float *p = pose + o * pose_stride, *k = K + o * 9;
    const double yd = (double)p[3];
    const float sy = (float)sin(yd), cy = (float)cos(yd);
    const float R[9] = { cy, 0.0f, sy, 0.0f, 1.0f, 0.0f, -sy, 0.0f, cy };
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s.pr[i * 3 + j] = k[i * 3 + 0] * R[0 * 3 + j] + k[i * 3 + 1] * R[1 * 3 + j] + k[i * 3 + 2] * R[2 * 3 + j];
        s.pt[i] = k[i * 3 + 0] * p[0] + k[i * 3 + 1] * p[1] + k[i * 3 + 2] * p[2];
    }
    s.umax = img[o * 2 + 1] + border;
    s.vmax = img[o * 2 + 0] + border;
    return s;
}

__global__ void __launch_bounds__(256) uncert_projection_kernel(const float *__restrict__ c3d, const float *__restrict__ pose,
                                                                long long pose_stride, const float *__restrict__ K, const float *__restrict__ img, long long total,
                                                                int hw, float z_min, float border, float *__restrict__ c2d) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long o = idx / hw, px = idx - o * hw;
    const ProjSetup s = proj_setup(pose, pose_stride, K, img, o, border);
    const float *x = c3d + o * 3 * hw + px;
    const float X = x[0], Y = x[hw], Z = x[2 * hw];
    const float pu = s.pr[0] * X + s.pr[1] * Y + s.pr[2] * Z + s.pt[0];
    const float pv = s.pr[3] * X + s.pr[4] * Y + s.pr[5] * Z + s.pt[1];
    const float pz = s.pr[6] * X + s.pr[7] * Y + s.pr[8] * Z + s.pt[2];
    const float zc = clamp_lo(pz, z_min);
    float *out = c2d + o * 2 * hw + px;
    out[0] = nan_min(clamp_lo(pu / zc, -border), s.umax);
    out[hw] = nan_min(clamp_lo(pv / zc, -border), s.vmax);
}

__global__ void __launch_bounds__(256) uncert_projection_backward_kernel(const float *__restrict__ c3d, const float *__restrict__ pose,
                                                                         long long pose_stride, const float *__restrict__ K, const float *__restrict__ img,
                                                                         long long total, int hw, float z_min, float border,
                                                                         const float *__restrict__ g2d, float *__restrict__ g3d) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long o = idx / hw, px = idx - o * hw;
    const ProjSetup s = proj_setup(pose, pose_stride, K, img, o, border);
    const float *x = c3d + o * 3 * hw + px;
    const float X = x[0], Y = x[hw], Z = x[2 * hw];
    const float pu = s.pr[0] * X + s.pr[1] * Y + s.pr[2] * Z + s.pt[0];
    const float pv = s.pr[3] * X + s.pr[4] * Y + s.pr[5] * Z + s.pt[1];
    const float pz = s.pr[6] * X + s.pr[7] * Y + s.pr[8] * Z + s.pt[2];
    const float zc = clamp_lo(pz, z_min);
    const float *g = g2d + o * 2 * hw + px;
    float gp[2];
    const float num[2] = { pu, pv }, hi[2] = { s.umax, s.vmax }, gin[2] = { g[0], g[hw] };
    float gz = 0.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float u0 = num[c] / zc, u1 = clamp_lo(u0, -border);
        // torch.min backward: grad / 2 at a tie, 0 where this side is the larger; then clamp(min) passes at its bound
        float gu = u1 == hi[c] ? gin[c] / 2.0f : (u1 > hi[c] ? 0.0f : gin[c]);
        gu = u0 >= -border ? gu : 0.0f;
        gp[c] = gu / zc;
        const float gzc = (-gu * num[c]) / (zc * zc);
        gz = c == 0 ? gzc : gz + gzc;
    }
    gz = pz >= z_min ? gz : 0.0f;
    float *gx = g3d + o * 3 * hw + px;
    gx[0] = s.pr[0] * gp[0] + s.pr[3] * gp[1] + s.pr[6] * gz;
    gx[hw] = s.pr[1] * gp[0] + s.pr[4] * gp[1] + s.pr[7] * gz;
    gx[2 * hw] = s.pr[2] * gp[0] + s.pr[5] * gp[1] + s.pr[8] * gz;
}

struct KlParams { int identity; float delta, half_delta, inv_max; };

// inverse std and the raw (undivided) per-element loss
__device__ __forceinline__ void robust_kl_elem(float x, float ls, const KlParams &p, float &inv, float &raw) {
#pragma clang fp contract(off)
    const float e = mr_expf(-ls);
    inv = e > p.inv_max ? p.inv_max : e;                                    // clamp(max=1/eps), NaN stays
    const float diff = p.identity ? x : fabsf(x);
    const float dw = diff * inv;
    raw = (dw < p.delta ? 0.5f * (dw * dw) : p.delta * (dw - p.half_delta)) + ls;
}

// all-reduce of two fp64 values over a 256-thread workgroup, fixed order (waves, then waves 0..3)
__device__ __forceinline__ void robust_kl_block_sum(double (&a)[2]) {
    __shared__ double red[4][2];
    wave_allreduce<2>(a);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = a[0]; red[wave][1] = a[1]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) a[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

__global__ void __launch_bounds__(256) robust_kl_partial_kernel(const float *__restrict__ pred, const float *__restrict__ logstd,
                                                                long long numel, KlParams p, double *__restrict__ partials) {
    double a[2] = { 0.0, 0.0 };
    for (long long i = (long long)blockIdx.x * kKlThreads + threadIdx.x; i < numel; i += (long long)gridDim.x * kKlThreads) {
        float inv, raw;
        robust_kl_elem(pred[i], logstd[i], p, inv, raw);
        a[0] += (double)inv;
        a[1] += (double)raw;
    }
    robust_kl_block_sum(a);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = a[0]; partials[2 * blockIdx.x + 1] = a[1]; }
}

__global__ void __launch_bounds__(256) robust_kl_fold_kernel(const double *__restrict__ partials, int nblocks, long long numel, int training,
                                                             float keep, float momentum, int mean, float loss_weight,
                                                             float *__restrict__ mean_inv_std, float *__restrict__ loss, float *__restrict__ c_out) {
#pragma clang fp contract(off)
    double a[2] = { 0.0, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += kKlThreads) { a[0] += partials[2 * b]; a[1] += partials[2 * b + 1]; }
    robust_kl_block_sum(a);
    if (threadIdx.x != 0) return;
    float m = mean_inv_std[0];
    if (training) {
        const float avg = (float)(a[0] / (double)numel);
        m = m * keep;
        m = m + momentum * avg;
        mean_inv_std[0] = m;
    }
    const float c = clamp_lo(m, 1e-6f);
    double s = a[1] / (double)c;
    if (mean) s = s / (double)numel;
    loss[0] = loss_weight * (float)s;
    c_out[0] = c;
}

__global__ void __launch_bounds__(256) robust_kl_backward_kernel(const float *__restrict__ pred, const float *__restrict__ logstd,
                                                                 long long numel, KlParams p, const float *__restrict__ grad_loss,
                                                                 const float *__restrict__ c_saved, float loss_weight, int mean,
                                                                 float *__restrict__ grad_pred, float *__restrict__ grad_logstd) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kKlThreads + threadIdx.x;
    if (i >= numel) return;
    // the chain of torch's backward: loss_weight *, mean (/ numel) or sum, div_(c)
    float g = grad_loss[0] * loss_weight;
    if (mean) g = g / (float)numel;
    g = g / c_saved[0];
    const float x = pred[i], ls = logstd[i];
    const float e = mr_expf(-ls);
    const float inv = e > p.inv_max ? p.inv_max : e;
    const float diff = p.identity ? x : fabsf(x);
    const float dw = diff * inv;
    const float gdw = dw < p.delta ? g * dw : g * p.delta;                  // dw == delta takes the linear branch, as torch.where does
    const float gdiff = gdw * inv, ginv = gdw * diff;
    // |x|: sgn(x) * grad, 0 at x == 0 (NaN stays NaN)
    grad_pred[i] = p.identity ? gdiff : (x > 0.0f ? gdiff : (x < 0.0f ? -gdiff : (x == 0.0f ? 0.0f : x)));
    const float ge = e <= p.inv_max ? ginv : 0.0f;                          // clamp(max) passes the gradient at its bound
    grad_logstd[i] = g + -(ge * e);
}
