// score_head_kernel.inc — N7 (DESIGN.md §13): MLPScoreHead.forward in eval mode, with the sigmoid, the mask of failed solves and the
// 2-D score multiply behind it (mlp_score_head.py:94-115, monorun_roi_head.py:544-550), as ONE launch.  The formula and the layout
// of `params` are the contract comment of mr_score_head_forward in include/monorun_heads.h.
//
// One 256-thread workgroup per tile of kScoreRows = 4 rows:
//   stage 0  threads 0..67 gather and normalise the 17 inputs of the tile's rows                      -> LDS xn[k][row]
//   stage 1  thread j (stride 256) owns channel j of the pose layer: 17 fmas per row from W1t (a wave's load is contiguous),
//            bias, relu, + reg_fc_out                                                                  -> LDS h1[k][row]
//   stage 2  the fused layer, 256 output channels per pass: lane l of every wave owns channels 4l..4l+3 of the pass (one 16-byte
//            load of W2t per k: a wave reads 1 KiB of one row), and the four waves split k into four contiguous quarters of
//            ceil(c1 / 4); every k costs one ds_read_b128 (h1 of the four rows, a broadcast) and 16 fmas.  The waves' partial sums
//            meet in LDS; thread t then owns channel t of the pass: ((p0 + p1) + p2) + p3, bias, relu, times w3, into its dot.
//   stage 3  the dot over the workgroup with wave_allreduce (fp64 adds of the 256 fp32 partials, fixed order), b3, sigmoid, mask,
//            2-D score; thread 0 stores the tile's scores.
// Rows of the last tile beyond n compute on zeros and store nothing.  Every row has its own accumulators from stage 0 on, so a
// NaN of one row never reaches another, and the order of a row's sums depends on c1 and c2 only.
// LDS: h1 32 KiB (c1 <= 2048) + partials 16 KiB + xn + the reduction's 128 bytes, static; no scratch.

constexpr int kScoreRows = 4;
constexpr int kScoreIn = 17;
constexpr int kScoreThreads = 256;

__host__ __device__ inline long long score_r4(long long v) { return (v + 3) / 4 * 4; }

struct ScoreLayout { long long w1t, b1, w2t, b2, w3, b3, numel; int c2p; };

__host__ __device__ inline ScoreLayout score_layout(int c1, int c2) {
    ScoreLayout l;
    l.c2p = (int)score_r4(c2);
    l.w1t = 64;
    l.b1 = l.w1t + score_r4((long long)kScoreIn * c1);
    l.w2t = l.b1 + score_r4(c1);
    l.b2 = l.w2t + (long long)c1 * l.c2p;
    l.w3 = l.b2 + l.c2p;
    l.b3 = l.w3 + l.c2p;
    l.numel = l.b3 + 4;
    return l;
}

struct ScoreArgs {
    const float *reg, *yaw, *t, *cov, *dim; long long reg_stride, yaw_stride, t_stride, dim_stride;
    const uint8_t *ret_val; const float *scores_2d, *params; int n, c1, c2, sigmoid; float *out;
};

__global__ void __launch_bounds__(kScoreThreads) score_head_forward_kernel(ScoreArgs a) {
    __shared__ __attribute__((aligned(16))) float s_h1[MR_SCORE_MAX_C1 * kScoreRows];
    __shared__ __attribute__((aligned(16))) float s_part[4 * kScoreRows * 256];
    __shared__ __attribute__((aligned(16))) float s_x[kScoreIn * kScoreRows];
    __shared__ double s_red[4][kScoreRows];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * kScoreRows;
    const int c1 = a.c1, c2 = a.c2;
    const ScoreLayout L = score_layout(c1, c2);
    const float *P = a.params;

    // stage 0: the 17-vector of every row, normalised
    if (tid < kScoreIn * kScoreRows) {
#pragma clang fp contract(off)
        const int r = tid / kScoreIn, k = tid - r * kScoreIn;
        const long long row = row0 + r;
        float xn = 0.0f;
        if (row < a.n) {
            // torch.tril_indices(4, 4): (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) (3,1) (3,2) (3,3)
            const int tri = k - 4, tr = tri < 1 ? 0 : (tri < 3 ? 1 : (tri < 6 ? 2 : 3)), tc = tri - tr * (tr + 1) / 2;
            float x;
            if (k == 0) x = a.yaw[row * a.yaw_stride];
            else if (k < 4) x = a.t[row * a.t_stride + (k - 1)];
            else if (k < 14) x = a.cov[row * 16 + tr * 4 + tc];
            else x = a.dim[row * a.dim_stride + (k - 14)];
            xn = (x - P[k]) * P[kScoreIn + k] + P[2 * kScoreIn + k];
        }
        s_x[k * kScoreRows + r] = xn;
    }
    __syncthreads();

    // stage 1: h1 = relu(W1 xn + b1) + reg_fc_out
    for (int j = tid; j < c1; j += kScoreThreads) {
        float acc[kScoreRows] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
        for (int k = 0; k < kScoreIn; ++k) {
            const float w = P[L.w1t + (long long)k * c1 + j];
            const float4 x = *reinterpret_cast<const float4 *>(&s_x[k * kScoreRows]);
            acc[0] = fmaf(w, x.x, acc[0]); acc[1] = fmaf(w, x.y, acc[1]); acc[2] = fmaf(w, x.z, acc[2]); acc[3] = fmaf(w, x.w, acc[3]);
        }
        const float b = P[L.b1 + j];
        float4 h;
        float *hp = &h.x;
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r) {
            const long long row = row0 + r;
            const float g = row < a.n ? a.reg[row * a.reg_stride + j] : 0.0f;
            hp[r] = clamp_lo(acc[r] + b, 0.0f) + g;
        }
        *reinterpret_cast<float4 *>(&s_h1[j * kScoreRows]) = h;
    }
    __syncthreads();

    // stage 2: h2 = relu(W2 h1 + b2), folded into the dot with w3 as it is produced
    const int kq = (c1 + 3) / 4;
    const int k0 = wave * kq < c1 ? wave * kq : c1, k1 = k0 + kq < c1 ? k0 + kq : c1;
    float dot[kScoreRows] = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (int jp = 0; jp < c2; jp += 256) {
        const int jb = jp + 4 * lane;                       // this lane's four channels of the pass
        float acc[4][kScoreRows];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < kScoreRows; ++r) acc[c][r] = 0.0f;
        if (jb < L.c2p) {
            const float *w2 = P + L.w2t + jb;
#pragma unroll 8
            for (int k = k0; k < k1; ++k) {
                const float4 w = *reinterpret_cast<const float4 *>(w2 + (long long)k * L.c2p);
                const float4 h = *reinterpret_cast<const float4 *>(&s_h1[k * kScoreRows]);
                const float wv[4] = { w.x, w.y, w.z, w.w }, hv[4] = { h.x, h.y, h.z, h.w };
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int r = 0; r < kScoreRows; ++r) acc[c][r] = fmaf(wv[c], hv[r], acc[c][r]);
            }
        }
        if (jp) __syncthreads();                            // the previous pass has read s_part
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r)
            *reinterpret_cast<float4 *>(&s_part[(wave * kScoreRows + r) * 256 + 4 * lane]) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        __syncthreads();
        const int j = jp + tid;
        if (j < c2) {
            const float b = P[L.b2 + j], w3 = P[L.w3 + j];
#pragma unroll
            for (int r = 0; r < kScoreRows; ++r) {
                const float s = ((s_part[(0 * kScoreRows + r) * 256 + tid] + s_part[(1 * kScoreRows + r) * 256 + tid]) +
                                 s_part[(2 * kScoreRows + r) * 256 + tid]) + s_part[(3 * kScoreRows + r) * 256 + tid];
                dot[r] = fmaf(clamp_lo(s + b, 0.0f), w3, dot[r]);
            }
        }
    }

    // stage 3: z = w3 . h2 + b3 over the workgroup, then the epilogue
    double d[kScoreRows] = { (double)dot[0], (double)dot[1], (double)dot[2], (double)dot[3] };
    wave_allreduce<kScoreRows>(d);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r) s_red[wave][r] = d[r];
    }
    __syncthreads();
    if (tid < kScoreRows && row0 + tid < a.n) {
#pragma clang fp contract(off)
        const long long row = row0 + tid;
        const float z = (float)(((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid]) + P[L.b3];
        float s = a.sigmoid ? 1.0f / (1.0f + mr_expf(-z)) : z;
        const bool failed = a.ret_val && !a.ret_val[row];
        s = failed ? 0.0f : s;
        if (a.scores_2d && !failed) s = s * a.scores_2d[row];
        a.out[row] = s;
    }
}
