// noc_target_kernel.inc — N9 (DESIGN.md §15): the NOC head's LiDAR supervision, the reference's _noc_forward_train
// (monorun/models/roi_heads/monorun_roi_head.py:343-365): NOCCoder.encode (core/bbox_3d/coord_coder/noc_coder.py:17-48) fused into
// masked_dense_target (core/bbox_3d/masked_dense_target.py), and SmoothL1LossMod (models/losses/smooth_l1_loss.py) forward and
// backward.  Included by monorun_pnp.hip inside its anonymous namespace, after projection_loss_kernel.inc (wave_allreduce, clamp_lo).
//
// Dense target, two launches, no memset, no atomics, nothing copied on the host but the per-image table (a kernel argument):
//   noc_dense_target_kernel: a workgroup per positive RoI, threads stride over the h w bins.  Per tap the sampling position and the
//   four bilinear weights are computed once (roi_bilinear's border rules and operation order), the four corner pixels of the three
//   coordinate planes and of the mask plane are read from the image's own tensors and ENCODED on the fly, per pixel and in fp32:
//     fg = m >= eps_c;  part_k = c_k / (m < eps_c ? eps_c : m) / (dim_k < eps_c ? eps_c : dim_k);  part_2 = -part_2 when flipped;
//     m' = fg ? m : 0;  enc_k = ((part_k - mean_k) / std_k) m'
//   blended w1 v1 + w2 v2 + w3 v3 + w4 v4, accumulated over the taps and divided by the tap count as roi_align_avg_bin does.  Bilinear
//   sampling reads the encoded map at integer pixels only, so this equals "encode the whole map, then RoIAlign it" bit for bit.
//   Then M = pooled m', wgt = M > eps_t, T_k = wgt ? T_k / M : T_k; the workgroup's number of positive bins goes to count[i].
//   noc_target_normalise_kernel: every workgroup adds the n integer counts (any order gives the same integer) and divides its RoI's
//   0/1 weights by c = max(fp32(total) / fp32(n h w), eps_t): torch's weights / mean(weights).clamp(min=eps) with the mean taken as
//   sum / numel (exact while n h w < 2^24, where an fp32 sum of ones is).
// SAFETY (the one deviation from the reference, which would index out of range): a RoI whose image index is outside [0, num_images),
// whose ground-truth index is outside [0, G_j) or whose clipped box has a non-finite coordinate reads nothing and gets zero targets,
// zero weights and count 0.  A finite clipped box lies in [0, W] x [0, H], so its tap counts are at most H and W, and every tap's
// corner indices are clamped into the map by the border rules: no input makes a loop unbounded or an address leave its tensor.
//
// Smooth L1 (mod): l = d < beta ? 0.5 d d / beta : d - fp32(0.5 beta), d = |pred - target|, times the element weight (absent, of
// pred's shape, or (n, 1, h, w) broadcast over the channels) in fp32; fp64 partial sums per thread, per workgroup to the workspace;
// a single workgroup folds the partials in a fixed order, divides by numel for 'mean' and writes fp32(loss_weight) * fp32(sum).
// Backward: one launch, one product chain per element in the order of torch's autograd.
// No scratch; 256-thread workgroups; results are ordinary vector stores; bitwise reproducible.

constexpr int kNocMaxImages = 32;           // per-image table entries a launch carries as a kernel argument
constexpr int kNocThreads = 256;

struct NocImage {
    const float *coords, *mask, *dims;      // (G, 3, H, W), (G, 1, H, W) contiguous; dims rows [l, h, w, ...] with a row stride
    long long dims_stride;
    int H, W, G, flip;
};

struct NocTargetArgs {
    NocImage img[kNocMaxImages];
    int num_images;
    const float *rois; const int *roi_img; const long long *roi_gt;
    int n, h, w;
    const float *means, *stds;
    float eps_c, eps_t;
    float *targets, *weights; int *counts;
};

// sum of one int over the 256 threads of a workgroup (every thread gets it)
__device__ __forceinline__ int noc_block_sum(int v) {
    __shared__ int red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

struct NocEnc { float dim[3], mean[3], std[3], eps_c; int flip; };

// the encoded pixel (three coordinate channels and the mask) at element offset o of its plane
__device__ __forceinline__ void noc_encode_pixel(const float *__restrict__ c, const float *__restrict__ m, long long plane, long long o,
                                                 const NocEnc &e, float (&v)[4]) {
#pragma clang fp contract(off)
    const float mk = m[o];
    const bool fg = mk >= e.eps_c;
    const float mc = clamp_lo(mk, e.eps_c);
    const float mp = fg ? mk : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float part = c[k * plane + o] / mc / e.dim[k];
        if (k == 2 && e.flip) part = -part;
        v[k] = ((part - e.mean[k]) / e.std[k]) * mp;
    }
    v[3] = mp;
}

// roi_bilinear over the four encoded planes: one position, one set of weights, 4 x 4 corner values
__device__ __forceinline__ void noc_bilinear4(const float *__restrict__ c, const float *__restrict__ m, int H, int W, float y, float x,
                                              const NocEnc &e, float (&out)[4]) {
#pragma clang fp contract(off)
    if (!(y >= -1.0f && y <= (float)H && x >= -1.0f && x <= (float)W)) { out[0] = out[1] = out[2] = out[3] = 0.0f; return; }
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
    if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
    const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
    const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
    const long long plane = (long long)H * W;
    float v1[4], v2[4], v3[4], v4[4];
    noc_encode_pixel(c, m, plane, (long long)y_low * W + x_low, e, v1);
    noc_encode_pixel(c, m, plane, (long long)y_low * W + x_high, e, v2);
    noc_encode_pixel(c, m, plane, (long long)y_high * W + x_low, e, v3);
    noc_encode_pixel(c, m, plane, (long long)y_high * W + x_high, e, v4);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = w1 * v1[k] + w2 * v2[k] + w3 * v3[k] + w4 * v4[k];
}

__device__ __forceinline__ float noc_clip(float v, float hi) { return clamp_hi(clamp_lo(v, 0.0f), hi); }      // clamp(0, hi), NaN stays
__device__ __forceinline__ bool noc_finite(float v) { return fabsf(v) <= 3.402823466e38f; }

__global__ void __launch_bounds__(256) noc_dense_target_kernel(const NocTargetArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x;
    const long long hw = (long long)a.h * a.w;      // 64-bit: 3 h w may pass 2^31 where n h w does not
    float *__restrict__ T = a.targets + i * 3 * hw;
    float *__restrict__ Wt = a.weights + i * hw;
    const int j = a.roi_img[i];
    const long long g = a.roi_gt[i];
    bool ok = j >= 0 && j < a.num_images;
    const NocImage &im = a.img[ok ? j : 0];
    const int H = im.H, W = im.W;
    ok = ok && g >= 0 && g < (long long)im.G;
    const float *r = a.rois + (long long)i * 4;
    const float x1 = noc_clip(r[0], (float)W), y1 = noc_clip(r[1], (float)H), x2 = noc_clip(r[2], (float)W), y2 = noc_clip(r[3], (float)H);
    ok = ok && noc_finite(x1) && noc_finite(y1) && noc_finite(x2) && noc_finite(y2);
    int cnt = 0;
    if (!ok) {
        for (long long p = threadIdx.x; p < hw; p += kNocThreads) { T[p] = 0.0f; T[hw + p] = 0.0f; T[2 * hw + p] = 0.0f; Wt[p] = 0.0f; }
    } else {
        NocEnc e;
        e.eps_c = a.eps_c; e.flip = im.flip;
#pragma unroll
        for (int k = 0; k < 3; ++k) { e.dim[k] = clamp_lo(im.dims[g * im.dims_stride + k], a.eps_c); e.mean[k] = a.means[k]; e.std[k] = a.stds[k]; }
        const long long plane = (long long)H * W;
        const float *__restrict__ c = im.coords + g * 3 * plane;
        const float *__restrict__ m = im.mask + g * plane;
        // roi_align_avg_bin's per-RoI terms: aligned, sampling_ratio 0, spatial_scale 1
        const float sw = x1 - 0.5f, sh = y1 - 0.5f;
        const float rw = (x2 - 0.5f) - sw, rh = (y2 - 0.5f) - sh;
        const float bh = rh / (float)a.h, bw = rw / (float)a.w;
        int gh = (int)ceilf(rh / (float)a.h), gw = (int)ceilf(rw / (float)a.w);
        gh = gh > H ? H : gh; gw = gw > W ? W : gw;                   // never taken: rh <= H and rw <= W for a clipped box
        const float count = (float)max(gh * gw, 1);
        for (int p = threadIdx.x; p < (int)hw; p += kNocThreads) {         // h w <= n h w <= 2^31 - 1
            const int ph = p / a.w, pw = p - ph * a.w;
            float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
            for (int iy = 0; iy < gh; ++iy) {
                const float y = sh + (float)ph * bh + ((float)iy + 0.5f) * bh / (float)gh;
                for (int ix = 0; ix < gw; ++ix) {
                    const float x = sw + (float)pw * bw + ((float)ix + 0.5f) * bw / (float)gw;
                    float v[4];
                    noc_bilinear4(c, m, H, W, y, x, e, v);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] += v[k];
                }
            }
            const float M = acc[3] / count;
            const bool pos = M > a.eps_t;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float t = acc[k] / count; T[k * hw + p] = pos ? t / M : t; }
            Wt[p] = pos ? 1.0f : 0.0f;
            cnt += pos ? 1 : 0;
        }
    }
    cnt = noc_block_sum(cnt);
    if (threadIdx.x == 0) a.counts[i] = cnt;
}

__global__ void __launch_bounds__(256) noc_target_normalise_kernel(const int *__restrict__ counts, int n, int hw, float eps_t,
                                                                   float *__restrict__ weights) {
#pragma clang fp contract(off)
    long long s = 0;
    for (int k = threadIdx.x; k < n; k += kNocThreads) s += counts[k];
    // n h w <= 2^31 - 1 (checked by the host), so the total fits an int and so does every partial
    const int total = noc_block_sum((int)s);
    const float mean = (float)total / (float)((long long)n * hw);
    const float c = clamp_lo(mean, eps_t);
    float *__restrict__ Wt = weights + (long long)blockIdx.x * hw;
    for (int p = threadIdx.x; p < hw; p += kNocThreads) Wt[p] = Wt[p] / c;
}

// ---- SmoothL1LossMod
struct Sl1Params { float beta, half_beta; int weight_mode; long long chw, hw; };      // weight_mode 0 none, 1 of pred's shape, 2 (n, 1, h, w)

__device__ __forceinline__ float sl1_weight(const float *__restrict__ weight, const Sl1Params &p, long long i) {
    if (p.weight_mode == 1) return weight[i];
    const long long o = i / p.chw;
    return weight[o * p.hw + (i - o * p.chw) % p.hw];
}

__device__ __forceinline__ double sl1_block_sum(double v) {
    __shared__ double red[4];
    double a[1] = { v };
    wave_allreduce<1>(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a[0];
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256) smooth_l1_mod_loss_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                                 const float *__restrict__ weight, long long numel, Sl1Params p,
                                                                 double *__restrict__ partials) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * kKlThreads + threadIdx.x; i < numel; i += (long long)gridDim.x * kKlThreads) {
        const float d = fabsf(pred[i] - target[i]);
        float l = d < p.beta ? 0.5f * d * d / p.beta : d - p.half_beta;
        if (p.weight_mode) l = l * sl1_weight(weight, p, i);
        acc += (double)l;
    }
    acc = sl1_block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) smooth_l1_mod_finish_kernel(const double *__restrict__ partials, int nblocks, long long numel, int mean,
                                                                   float loss_weight, float *__restrict__ loss) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kKlThreads) acc += partials[b];
    acc = sl1_block_sum(acc);
    if (threadIdx.x != 0) return;
    if (mean) acc = acc / (double)numel;
    loss[0] = loss_weight * (float)acc;
}

__global__ void __launch_bounds__(256) smooth_l1_mod_loss_backward_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                                          const float *__restrict__ weight, long long numel, Sl1Params p,
                                                                          const float *__restrict__ grad_loss, float loss_weight, int mean,
                                                                          float *__restrict__ grad_pred) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kKlThreads + threadIdx.x;
    if (i >= numel) return;
    // the chain of torch's backward: loss_weight *, mean (/ numel) or sum, * weight, where, the branch, abs
    float g = grad_loss[0] * loss_weight;
    if (mean) g = g / (float)numel;
    if (p.weight_mode) g = g * sl1_weight(weight, p, i);
    const float x = pred[i] - target[i];
    const float d = fabsf(x);
    float gd;
    if (d < p.beta) {
        const float gb = g / p.beta;                                  // (0.5 d) d / beta: both factors of the product carry d
        gd = (gb * d) * 0.5f + gb * (0.5f * d);
    } else {
        gd = g;
    }
    grad_pred[i] = x > 0.0f ? gd : (x < 0.0f ? -gd : (x == 0.0f ? 0.0f : x));      // sgn(x) * grad, 0 at x == 0 (NaN stays NaN)
}
