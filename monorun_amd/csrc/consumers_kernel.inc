// consumers_kernel.inc — the small kernels around the PnP (included by monorun_pnp.hip inside its anonymous namespace, after kitti_eval_kernel.inc):
// RoIAlign (its bin samplers: noc_decode_kernel.inc), the rotated-BEV NMS, the spin kernel and the covariance fallback's eigenvalue rule.
__global__ void __launch_bounds__(256) roi_align_avg_kernel(const float *in, const float *rois, int K, int C, int H, int W, int out_h, int out_w,
                                                            float spatial_scale, int sampling_ratio, int aligned, float *out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)K * C * out_h * out_w) return;
    const int pw = (int)(idx % out_w), ph = (int)((idx / out_w) % out_h), c = (int)((idx / ((long long)out_w * out_h)) % C);
    const int n = (int)(idx / ((long long)out_w * out_h * C));
    const float *r = rois + (long long)n * 5;
    const int bi = (int)r[0];
    out[idx] = roi_align_avg_bin(in + ((long long)bi * C + c) * H * W, H, W, r[1] * spatial_scale, r[2] * spatial_scale, r[3] * spatial_scale,
                                 r[4] * spatial_scale, ph, pw, out_h, out_w, sampling_ratio, aligned);
}

// ------------------------------------------------------------------------------------------------
// N1: rotated-BEV NMS, the consumer that follows the PnP (monorun_roi_head.py:619-655 calls
// mmdet3d.ops.iou3d.nms_gpu — third-party, not in the reference tree; restated from its published algorithm:
// sort by score, rotated-rectangle IoU = overlap / max(area_a + area_b - overlap, 1e-8), greedy
// suppression of IoU > thr).  One workgroup per class group (n <= kNmsMax boxes).
constexpr int kNmsMax = 512;

#define MR_NMS_FN __device__ __forceinline__
#include "nms_order.inc"
#undef MR_NMS_FN

struct NmsBox { float cx, cy; float px[4], py[4]; float area; };   // CCW corners relative to nothing (absolute)

__device__ __forceinline__ float rotated_iou(const NmsBox &a, const NmsBox &b) {
    // a box of zero area (a segment, a point) meets nothing in a set of positive area: IoU 0.  Its zero-length edges clip nothing, so
    // the boundary sum below would count the other box whole.  A NaN area (a NaN coordinate) compares false: IoU 0 as well.
    if (!(a.area > 0.0f && b.area > 0.0f)) return 0.0f;
    // work relative to a's centre to keep fp32 cancellation small
    float ax[4], ay[4], bx[4], by[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ax[i] = a.px[i] - a.cx; ay[i] = a.py[i] - a.cy; bx[i] = b.px[i] - a.cx; by[i] = b.py[i] - a.cy; }
    float ov = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ov += edge_inside_area_t<float, true>(ax[i], ay[i], ax[(i + 1) & 3], ay[(i + 1) & 3], bx, by);
        ov += edge_inside_area_t<float, false>(bx[i], by[i], bx[(i + 1) & 3], by[(i + 1) & 3], ax, ay);
    }
    ov = fmaxf(ov, 0.0f);
    return ov / fmaxf(a.area + b.area - ov, 1e-8f);
}

// The box record of one [x1, y1, x2, y2, angle] row: every kernel that runs the NMS builds its boxes here.
__device__ __forceinline__ NmsBox nms_make_box(float x1, float y1, float x2, float y2, float ang) {
    NmsBox nb;
    nb.cx = 0.5f * (x1 + x2); nb.cy = 0.5f * (y1 + y2);
    const float hw = 0.5f * (x2 - x1), hh = 0.5f * (y2 - y1);
    float sn, cs; sincosf(ang, &sn, &cs);
    const float ddx[4] = { -hw, hw, hw, -hw }, ddy[4] = { -hh, -hh, hh, hh };
#pragma unroll
    for (int c = 0; c < 4; ++c) { nb.px[c] = nb.cx + ddx[c] * cs + ddy[c] * sn; nb.py[c] = nb.cy - ddx[c] * sn + ddy[c] * cs; }
    if (hw * hh < 0.0f) {                               // keep the corner order counter-clockwise
        const float tx = nb.px[1], ty = nb.py[1]; nb.px[1] = nb.px[3]; nb.py[1] = nb.py[3]; nb.px[3] = tx; nb.py[3] = ty;
    }
    nb.area = fabsf((x2 - x1) * (y2 - y1));
    return nb;
}

// LDS of one group of n boxes (np2 = mr_nms_padded(n)): keys and indices of the sort, the boxes in sorted order, the suppression bits
// and 16 spare bytes.  include/monorun_result3d.h states the same sum with a fourth array.
__host__ __device__ constexpr size_t nms_group_lds(int n, int np2) {
    return (size_t)np2 * 8 + (size_t)n * sizeof(NmsBox) + (size_t)n * ((n + 31) / 32) * 4 + 16;
}

// One group's NMS over LDS, by the 256 threads of a block (n >= 1, uniform; `scores`: the group's n scores, any address space):
// the sort into nms_order.inc's order, the boxes (`box_of(j)`: the record of the group's box j), the suppression bits and the
// wave-synchronous greedy scan.  Thread 0 calls `emit(k, i)` for the k-th kept box, the one at sorted place i (sidx[i]: its index in
// the group).  Returns the number kept in the first wave (tid < 64) and 0 elsewhere; the caller's LDS writes of the scan are not
// yet visible to the other waves.
template <class BoxOf, class Emit>
__device__ __forceinline__ int nms_group_lds_scan(float *skey, int *sidx, NmsBox *sbox, unsigned *srow, int n, int np2, const float *scores,
                                                  float thr, int tid, BoxOf box_of, Emit emit) {
    const int nw = (n + 31) >> 5;
    for (int i = tid; i < np2; i += 256) mr_nms_fill(skey, sidx, i, n, scores);
    __syncthreads();
    // bitonic sort into the order of nms_order.inc: descending score, ties by ascending index, NaN scores last, padding after them —
    // so the first n places hold a permutation of 0 .. n-1 whatever the scores are
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += 256) mr_nms_step(skey, sidx, i, j, k);
            __syncthreads();
        }
    for (int i = tid; i < n; i += 256) sbox[i] = box_of(sidx[i]);
    __syncthreads();
    for (int t = tid; t < n * nw; t += 256) {
        const int i = t / nw, w = t - i * nw;
        unsigned bits = 0;
        const NmsBox a = sbox[i];
        for (int jj = 0; jj < 32; ++jj) {
            const int j = w * 32 + jj;
            if (j > i && j < n && rotated_iou(a, sbox[j]) > thr) bits |= 1u << jj;
        }
        srow[t] = bits;
    }
    __syncthreads();
    int kept = 0;
    if (tid < 64) {                                          // one wave, wave-synchronous greedy pass
        unsigned removed = 0;                                // lane w holds word w of the removed set (nw <= 16)
        for (int i = 0; i < n; ++i) {
            const unsigned word = __builtin_amdgcn_readlane(removed, i >> 5);
            if (!((word >> (i & 31)) & 1u)) {
                if (tid == 0) emit(kept, i);
                ++kept;
                if (tid < nw) removed |= srow[i * nw + tid];
            }
        }
    }
    return kept;
}

__global__ void __launch_bounds__(256) nms_bev_kernel(const float *boxes, const float *scores, const int *offsets, float thr,
                                                      long long *keep, int *num_keep) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int off = offsets[g], n = offsets[g + 1] - off;
    extern __shared__ __align__(16) unsigned char smem[];
    const int np2 = mr_nms_padded(n);
    float *skey = (float *)smem;                         // [np2]
    int *sidx = (int *)(skey + np2);                     // [np2]
    NmsBox *sbox = (NmsBox *)(sidx + np2);               // [n] in sorted order
    unsigned *srow = (unsigned *)(sbox + n);             // [n][(n + 31) / 32] suppression bits (j > i, IoU > thr)
    if (n <= 0) { if (tid == 0) num_keep[g] = 0; return; }
    const int kept = nms_group_lds_scan(
        skey, sidx, sbox, srow, n, np2, scores + off, thr, tid,
        [&](int j) { const float *b = boxes + (long long)(off + j) * 5; return nms_make_box(b[0], b[1], b[2], b[3], b[4]); },
        [&](int k, int i) { keep[off + k] = (long long)sidx[i]; });
    if (tid == 0) num_keep[g] = kept;
}

__global__ void __launch_bounds__(64) spin_kernel(long long ticks) {
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// The reference's covariance fallback (pnp_uncert.py:77-85), per object: when torch.inverse raises, the reference keeps an
// object only if the smallest eigenvalue of its Hessian exceeds max(1e-6 * largest, 0), and sets the others to h := I.  The fused
// kernel reports "Cholesky failed" instead; this optional pass applies the eigenvalue rule to every object.  The eigenvalues of
// cov = h^-1 are the reciprocals of h's, so the rule reads lambda_min(cov) > max(1e-6 * lambda_max(cov), 0) on the matrix the
// kernel already wrote (cyclic Jacobi on the 4x4, fp64).  One thread per object.
__global__ void __launch_bounds__(64) cov_symeig_rule_kernel(uint8_t *valid, float *cov, int B, float *lam_out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double A[16];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) { A[i] = (double)cov[(long long)b * 16 + i]; finite = finite && isfinite(A[i]); }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i + 1; j < 4; ++j) { const double m = 0.5 * (A[4 * i + j] + A[4 * j + i]); A[4 * i + j] = A[4 * j + i] = m; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dia += A[5 * i] * A[5 * i];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += A[4 * i + j] * A[4 * i + j];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[4 * p + q];
                if (apq != 0.0) {
                    const double theta = (A[5 * q] - A[5 * p]) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double x = A[4 * k + p], y = A[4 * k + q]; A[4 * k + p] = c * x - sn * y; A[4 * k + q] = sn * x + c * y; }
#pragma unroll
                    for (int k = 0; k < 4; ++k) { const double x = A[4 * p + k], y = A[4 * q + k]; A[4 * p + k] = c * x - sn * y; A[4 * q + k] = sn * x + c * y; }
                }
            }
    }
    const double lmin = fmin(fmin(A[0], A[5]), fmin(A[10], A[15])), lmax = fmax(fmax(A[0], A[5]), fmax(A[10], A[15]));
    if (lam_out) { lam_out[(long long)b * 2] = (float)lmin; lam_out[(long long)b * 2 + 1] = (float)lmax; }
    const bool keep = finite && (lmin > fmax(1e-6 * lmax, 0.0));
    if (!keep) {
        valid[b] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) cov[(long long)b * 16 + i] = (i % 5 == 0) ? 1.0f : 0.0f;
    }
}
