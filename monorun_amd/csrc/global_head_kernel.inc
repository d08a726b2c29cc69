// global_head_kernel.inc — N9 (DESIGN.md §16): FCExtractorMonteCarlo.forward in eval mode (fc_extractor_monte_carlo.py:41-63) with explicit
// dropout masks, the first layer factored over the channel mask.  The formulas, the mask layout and the workspace are the contract
// comment of mr_global_head_mc_forward in include/monorun_global.h.
//
// RoIs are processed in chunks of kGhChunk; a chunk is five launches:
//   gh_p_kernel      P[i,c,o]  = sum_k x[i,c,k] W1[o, cA + k]                                  batched over c   M = RoIs, K = A,  N = F
//   gh_h1_kernel     h1[s,i,o] = keep1 q1 relu(b1[o] + q0 sum_c keep0[s,i,c] P[i,c,o])         batched over i   M = S,    K = C,  N = F
//   gh_h2_kernel     h2[s,i,o] = keep2 q1 relu(b2[o] + sum_k W2[o,k] h1[s,i,k])                                 M = S RoIs, K = N = F
//   gh_out_kernel    y[s,i,j]  = bR[j] + sum_k WR[j,k] h2[s,i,k]                               one wave per sample row, VALU
//   gh_stats_kernel  mean, unbiased two-pass var of y over s and the mean of h2 over s, fp64 sums, each rounded once
// The first three are ONE tile routine, gh_mfma_tile, with functors for the A load, the B load and the epilogue: a 64 x 64 output
// tile per 256-thread workgroup, each of the four waves one 32 x 32 accumulator of v_mfma_f32_32x32x2_f32, K in steps of 32 through
// LDS (row stride 33 floats: the operand reads of a wave, 32 rows apart by 33, meet no bank twice), the next step's global loads in
// flight in registers while the current one multiplies.  K tails are zeros in LDS (0 * 0 added to the chain changes nothing); M and
// N tails are masked in the epilogue.  An output element is one fmaf chain in ascending k (the MFMA's definition), so its bits
// depend on the layer sizes only: not on n, on the RoI's position, on the chunking or on the tile it falls in.
// No atomics, no split-K, nothing allocated; LDS 2 * 64 * 33 * 4 = 16896 bytes static in the three tile kernels, none in the others.

constexpr int kGhBM = 64, kGhBN = 64, kGhBK = 32, kGhLd = kGhBK + 1, kGhThreads = 256;
constexpr int kGhChunk = 64;            // RoIs per pass: one M tile of gh_p_kernel, and the bound of the workspace
constexpr int kGhOutRows = 4;           // sample rows per workgroup of gh_out_kernel (one per wave)

typedef float gh_f32x16 __attribute__((ext_vector_type(16)));

struct GhArgs {
    const float *x, *w1, *b1, *w2, *b2, *wr, *br;
    const uint8_t *keep0, *keep1, *keep2;
    float q0, q1;
    int n, C, A, F, J, S;               // RoIs of the call, in_channels, roi area, fc channels, output width, samples
    int i0, nc;                         // this pass: RoIs [i0, i0 + nc)
    float *P, *h1, *h2, *ys;            // workspace: (nc, C, F), (S, nc, F), (S, nc, F), (S, nc, J)
    float *mean, *var, *reg, *samples;
};

// A(m, k), m < M, k < K: K contiguous in memory.  B(k, n): K contiguous (kNContig = false) or N contiguous (true); the flag picks the
// thread-to-element map of the global loads so that a wave's load is contiguous either way.  EP(m, n, acc) stores one element.
template <class AL, class BL, class EP>
__device__ __forceinline__ void gh_mfma_tile(const AL &al, const BL &bl, const EP &ep, int M, int N, int K, int m0, int n0,
                                             float *s_a, float *s_b) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int lk = tid & 31, lr = tid >> 5;                 // K-contiguous loads: column lk of rows lr + 8 j
    const int bn = tid & 63, bk = tid >> 6;                 // N-contiguous loads of B: column bn of k rows bk + 4 j
    float ra[8], rb[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = m0 + lr + 8 * j, k = k0 + lk;
            ra[j] = (m < M && k < K) ? al(m, k) : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = BL::kNContig ? n0 + bn : n0 + lr + 8 * j, k = BL::kNContig ? k0 + bk + 4 * j : k0 + lk;
            rb[j] = (n < N && k < K) ? bl(k, n) : 0.0f;
        }
    };
    gh_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float *pa = s_a + (wm + (lane & 31)) * kGhLd + (lane >> 5);
    const float *pb = s_b + (wn + (lane & 31)) * kGhLd + (lane >> 5);
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kGhBK) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s_a[(lr + 8 * j) * kGhLd + lk] = ra[j];
            if (BL::kNContig) s_b[bn * kGhLd + bk + 4 * j] = rb[j];
            else s_b[(lr + 8 * j) * kGhLd + lk] = rb[j];
        }
        __syncthreads();
        if (k0 + kGhBK < K) fetch(k0 + kGhBK);
        if (K - k0 >= kGhBK) {
#pragma unroll
            for (int kk = 0; kk < kGhBK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
        } else {
            for (int kk = 0; kk < K - k0; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[kk], pb[kk], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int n = n0 + wn + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M && n < N) ep(m, n, acc[r]);
    }
}

// ---- stage 1: P, batched over the channel c = blockIdx.z
struct GhPA {
    static constexpr bool kNContig = false;
    const float *x; long long row, off;                     // x[(i0 + m) * C * A + c * A + k]
    __device__ __forceinline__ float operator()(int m, int k) const { return x[m * row + off + k]; }
};
struct GhPB {
    static constexpr bool kNContig = false;
    const float *w; long long row, off;                     // W1[o * C * A + c * A + k]
    __device__ __forceinline__ float operator()(int k, int n) const { return w[n * row + off + k]; }
};
struct GhPE {
    float *P; long long row, off;                           // P[m * C * F + c * F + o]
    __device__ __forceinline__ void operator()(int m, int n, float acc) const { P[m * row + off + n] = acc; }
};

__global__ void __launch_bounds__(kGhThreads) gh_p_kernel(GhArgs a) {
    __shared__ float s_a[kGhBM * kGhLd];
    __shared__ float s_b[kGhBN * kGhLd];
    const long long c = blockIdx.z, ca = (long long)a.C * a.A;
    const GhPA al = { a.x + (long long)a.i0 * ca, ca, c * a.A };
    const GhPB bl = { a.w1, ca, c * a.A };
    const GhPE ep = { a.P, (long long)a.C * a.F, c * a.F };
    gh_mfma_tile(al, bl, ep, a.nc, a.F, a.A, blockIdx.y * kGhBM, blockIdx.x * kGhBN, s_a, s_b);
}

// ---- stage 2: h1, batched over the RoI of the pass ic = blockIdx.z; the A operand is the channel mask as 0.0 / 1.0
struct GhH1A {
    static constexpr bool kNContig = false;
    const uint8_t *keep; long long row;                     // keep0[(s * n + i) * C + c]
    __device__ __forceinline__ float operator()(int m, int k) const { return keep[m * row + k] ? 1.0f : 0.0f; }
};
struct GhH1B {
    static constexpr bool kNContig = true;
    const float *P; int F;                                  // P[ic][c][o]
    __device__ __forceinline__ float operator()(int k, int n) const { return P[(long long)k * F + n]; }
};
// keep q relu(b + scale acc): relu keeps NaN, and a dropped element of a NaN row stays NaN (NaN * 0), as torch's sequence has it
__device__ __forceinline__ float gh_act(float acc, float scale, float b, uint8_t keep, float q) {
#pragma clang fp contract(off)
    return clamp_lo(b + scale * acc, 0.0f) * (keep ? q : 0.0f);
}
struct GhH1E {
    float *h; const uint8_t *keep; const float *b; float q0, q1; long long hrow, krow;      // row m = sample s of this workgroup's RoI
    __device__ __forceinline__ void operator()(int m, int n, float acc) const {
        h[m * hrow + n] = gh_act(acc, q0, b[n], keep[m * krow + n], q1);
    }
};

__global__ void __launch_bounds__(kGhThreads) gh_h1_kernel(GhArgs a) {
    __shared__ float s_a[kGhBM * kGhLd];
    __shared__ float s_b[kGhBN * kGhLd];
    const int ic = blockIdx.z;
    const long long i = a.i0 + ic;
    const GhH1A al = { a.keep0 + i * a.C, (long long)a.n * a.C };
    const GhH1B bl = { a.P + (long long)ic * a.C * a.F, a.F };
    // row m = sample s: h1[(s * nc + ic) * F + o], keep1[(s * n + i) * F + o]
    const GhH1E ep = { a.h1 + (long long)ic * a.F, a.keep1 + i * a.F, a.b1, a.q0, a.q1, (long long)a.nc * a.F, (long long)a.n * a.F };
    gh_mfma_tile(al, bl, ep, a.S, a.F, a.C, blockIdx.y * kGhBM, blockIdx.x * kGhBN, s_a, s_b);
}

// ---- stage 3: h2 over all S * nc sample rows of the pass
struct GhH2A {
    const float *h; int F;
    __device__ __forceinline__ float operator()(int m, int k) const { return h[(long long)m * F + k]; }
};
struct GhH2B {
    static constexpr bool kNContig = false;
    const float *w; int F;                                  // W2[o * F + k]
    __device__ __forceinline__ float operator()(int k, int n) const { return w[(long long)n * F + k]; }
};

struct GhH2E {
    float *h; const uint8_t *keep; const float *b; float q1; int F, nc, n, i0;
    __device__ __forceinline__ void operator()(int m, int nn, float acc) const {
        const long long kr = (long long)(m / nc) * n + i0 + m % nc;
        h[(long long)m * F + nn] = gh_act(acc, 1.0f, b[nn], keep[kr * F + nn], q1);
    }
};

__global__ void __launch_bounds__(kGhThreads) gh_h2_kernel(GhArgs a) {
    __shared__ float s_a[kGhBM * kGhLd];
    __shared__ float s_b[kGhBN * kGhLd];
    const GhH2A al = { a.h1, a.F };
    const GhH2B bl = { a.w2, a.F };
    // row m = s * nc + ic: h2[m * F + o], keep2[(s * n + i0 + ic) * F + o]
    const GhH2E ep = { a.h2, a.keep2, a.b2, a.q1, a.F, a.nc, a.n, a.i0 };
    gh_mfma_tile(al, bl, ep, a.S * a.nc, a.F, a.F, blockIdx.y * kGhBM, blockIdx.x * kGhBN, s_a, s_b);
}

// ---- stage 4: the output layer, one wave per sample row: lane l owns k = l, l + 64, ... (an fmaf chain in ascending k), the 64
// partials meet in wave_allreduce (fp64 adds in a fixed order), the sum is rounded to fp32 and the bias added.  Four outputs a pass.
__global__ void __launch_bounds__(64 * kGhOutRows) gh_out_kernel(GhArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long m = (long long)blockIdx.x * kGhOutRows + wave;
    if (m >= (long long)a.S * a.nc) return;
    const int s = (int)(m / a.nc), ic = (int)(m % a.nc);
    const float *h = a.h2 + m * a.F;
    for (int j0 = 0; j0 < a.J; j0 += 4) {
        const float *w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = a.wr + (long long)(j0 + e < a.J ? j0 + e : a.J - 1) * a.F;
        float p[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int k = lane; k < a.F; k += 64) {
            const float hv = h[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = fmaf(w[e][k], hv, p[e]);
        }
        double d[4] = { (double)p[0], (double)p[1], (double)p[2], (double)p[3] };
        wave_allreduce<4>(d);
        if (lane < 4 && j0 + lane < a.J) {
            const int j = j0 + lane;
            const float y = (float)(lane == 0 ? d[0] : lane == 1 ? d[1] : lane == 2 ? d[2] : d[3]) + a.br[j];
            a.ys[m * a.J + j] = y;
            if (a.samples) a.samples[((long long)s * a.n + a.i0 + ic) * a.J + j] = y;
        }
    }
}

// One workgroup per RoI of the pass; thread t owns columns t, t + 256, ... of [y (J) | h2 (F)]: sequential fp64 sums over s.
__global__ void __launch_bounds__(256) gh_stats_kernel(GhArgs a) {
    const int ic = blockIdx.x;
    const long long i = a.i0 + ic;
    for (int col = threadIdx.x; col < a.J + a.F; col += 256) {
        const bool is_y = col < a.J;
        const int c = is_y ? col : col - a.J, width = is_y ? a.J : a.F;
        const float *src = (is_y ? a.ys : a.h2) + (long long)ic * width + c;
        const long long step = (long long)a.nc * width;
        double sum = 0.0;
        for (int s = 0; s < a.S; ++s) sum += (double)src[s * step];
        const double mu = sum / (double)a.S;
        if (!is_y) { a.reg[i * a.F + c] = (float)mu; continue; }
        double ss = 0.0;
        for (int s = 0; s < a.S; ++s) { const double dlt = (double)src[s * step] - mu; ss += dlt * dlt; }
        a.mean[i * a.J + c] = (float)mu;
        a.var[i * a.J + c] = (float)(ss / (double)(a.S - 1));
    }
}
