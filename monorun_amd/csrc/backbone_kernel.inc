// backbone_kernel.inc — the backbone's frozen-statistics batch norm fused with the residual add and the ReLU, its backward, and the stem's
// norm + ReLU + 3x3 / stride-2 max pooling (DESIGN.md section 23; included by monorun_pnp.hip inside its anonymous namespace).
// include/monorun_backbone.h defines the ops and the order of the two per-channel sums; contraction is off, every operation is an fp32
// one rounded on its own.
constexpr int kBnThreads = 256;         // MR_BN_THREADS
constexpr int kBnWaves = kBnThreads / 64;       // MR_BN_WAVES
constexpr int kBnChunk = 4096;          // MR_BN_CHUNK
constexpr int kBnRounds = kBnChunk / (4 * kBnThreads);        // groups of four per lane and chunk at the most
constexpr int kBnMaxGrid = 2048;        // MR_BN_MAX_GRID
constexpr int kBnFinalThreads = 64;     // MR_BN_FINAL_THREADS
constexpr int kStemTileH = 8, kStemTileW = 64;  // MR_STEM_TILE_H, MR_STEM_TILE_W: of the pooled map
constexpr int kStemThreads = 256;       // MR_STEM_THREADS
constexpr int kStemRows = 2 * kStemTileH + 1, kStemCols = 2 * kStemTileW + 1;
constexpr int kStemStage = (kStemRows * kStemCols + kStemThreads - 1) / kStemThreads;      // staged elements per lane

struct BnArgs {
    const float *x, *r, *g, *y_in;      // forward: x, r; backward: g, y_in (the saved y), x
    const float *mean, *var, *weight, *bias;
    float *y, *gx, *gr;                 // forward: y; backward: grad_x, grad_r
    float *part;                        // backward with parameter gradients: [2][chunks] partials, the bias sums first
    float *gw, *gb;                     // finalise
    int C, HW, chunks_per_plane, chunks, N;
    float eps;
    unsigned vec;                       // bit i: pointer i of the launch is 16-byte aligned (kBnVec*)
};
enum : unsigned { kBnVecX = 1, kBnVecR = 2, kBnVecY = 4, kBnVecG = 8, kBnVecGx = 16, kBnVecGr = 32, kBnVecYin = 64 };

// four consecutive floats whose index in the tensor is a multiple of 4: one 16-byte access where the pointer allows it
__device__ __forceinline__ float4 bn_load4(const float *p, bool vec) {
    if (vec) return *(const float4 *)p;
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void bn_store4(float *p, bool vec, float4 v) {
    if (vec) { *(float4 *)p = v; return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

// the per-channel constants of a chunk
struct BnChannel { float mean, istd, w, b, k; bool has_w, has_b; };
__device__ __forceinline__ BnChannel bn_channel(const BnArgs &a, int c) {
#pragma clang fp contract(off)
    BnChannel ch;
    ch.mean = a.mean[c];
    ch.istd = 1.0f / sqrtf(a.var[c] + a.eps);
    ch.has_w = a.weight != nullptr; ch.has_b = a.bias != nullptr;
    ch.w = ch.has_w ? a.weight[c] : 1.0f;
    ch.b = ch.has_b ? a.bias[c] : 0.0f;
    ch.k = ch.has_w ? ch.istd * ch.w : ch.istd;
    return ch;
}

__device__ __forceinline__ float bn_affine(const BnChannel &ch, float x) {
#pragma clang fp contract(off)
    float t = (x - ch.mean) * ch.istd;
    if (ch.has_w) t = t * ch.w;
    if (ch.has_b) t = t + ch.b;
    return t;
}

template <bool HAS_R, bool RELU>
__device__ __forceinline__ float bn_act_one(const BnChannel &ch, float x, float r) {
#pragma clang fp contract(off)
    float u = bn_affine(ch, x);
    if (HAS_R) u = u + r;
    if (RELU) u = u <= 0.0f ? 0.0f : u;
    return u;
}

// the chunk `q` of the launch: its first element's index in the tensor, its length and its channel.  One division per chunk, uniform.
struct BnSpan { int f0, n, c, head, groups; };
__device__ __forceinline__ BnSpan bn_span(const BnArgs &a, int q) {
    const int plane = q / a.chunks_per_plane, k = q - plane * a.chunks_per_plane;
    BnSpan s;
    s.c = plane % a.C;
    const int start = k * kBnChunk;
    s.n = min(kBnChunk, a.HW - start);
    s.f0 = plane * a.HW + start;                // < 2^31: the host has checked
    s.head = min((4 - (s.f0 & 3)) & 3, s.n);
    s.groups = (s.n - s.head) >> 2;
    return s;
}

// ------------------------------------------------------------------------------------------------ forward
template <bool HAS_R, bool RELU>
__global__ void __launch_bounds__(kBnThreads) bn_act_forward_kernel(const BnArgs a) {
#pragma clang fp contract(off)
    const bool vx = a.vec & kBnVecX, vr = a.vec & kBnVecR, vy = a.vec & kBnVecY;
    for (int q = blockIdx.x; q < a.chunks; q += gridDim.x) {
        const BnSpan s = bn_span(a, q);
        const BnChannel ch = bn_channel(a, s.c);
        const int t = threadIdx.x;
        if (t < s.head) {
            const int e = s.f0 + t;
            a.y[e] = bn_act_one<HAS_R, RELU>(ch, a.x[e], HAS_R ? a.r[e] : 0.0f);
        }
        const int body = s.f0 + s.head;
        // every load of the lane's (at most kBnRounds) groups is issued before the first is used; a lane past the last group of a round
        // loads that group again and stores nothing.  The rounds are uniform branches.
        float4 x[kBnRounds], r[kBnRounds];
#pragma unroll
        for (int j = 0; j < kBnRounds; ++j)
            if (j * kBnThreads < s.groups) {
                const int e = body + 4 * min(t + j * kBnThreads, s.groups - 1);
                x[j] = bn_load4(a.x + e, vx);
                if (HAS_R) r[j] = bn_load4(a.r + e, vr);
            }
#pragma unroll
        for (int j = 0; j < kBnRounds; ++j) {
            const int v = t + j * kBnThreads;
            if (v < s.groups) {
                float4 y;
                y.x = bn_act_one<HAS_R, RELU>(ch, x[j].x, HAS_R ? r[j].x : 0.0f);
                y.y = bn_act_one<HAS_R, RELU>(ch, x[j].y, HAS_R ? r[j].y : 0.0f);
                y.z = bn_act_one<HAS_R, RELU>(ch, x[j].z, HAS_R ? r[j].z : 0.0f);
                y.w = bn_act_one<HAS_R, RELU>(ch, x[j].w, HAS_R ? r[j].w : 0.0f);
                bn_store4(a.y + body + 4 * v, vy, y);
            }
        }
        const int tail = body + 4 * s.groups + t;
        if (tail < s.f0 + s.n) a.y[tail] = bn_act_one<HAS_R, RELU>(ch, a.x[tail], HAS_R ? a.r[tail] : 0.0f);
    }
}

// ------------------------------------------------------------------------------------------------ backward
// the butterfly of the header's step 2 over a wave
__device__ __forceinline__ float bn_wave_sum(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// one element: gm, the stores that are asked for, and the two terms added to the lane's accumulators
template <bool RELU, bool PARAMS>
__device__ __forceinline__ float bn_bwd_one(const BnChannel &ch, float g, float y, float x, float &sb, float &sw) {
#pragma clang fp contract(off)
    const float gm = RELU ? (y <= 0.0f ? 0.0f : g) : g;
    if (PARAMS) {
        const float xhat = (x - ch.mean) * ch.istd;
        const float term = gm * xhat;
        sb = sb + gm;
        sw = sw + term;
    }
    return gm;
}

template <bool RELU, bool PARAMS>
__global__ void __launch_bounds__(kBnThreads) bn_act_backward_kernel(const BnArgs a) {
#pragma clang fp contract(off)
    __shared__ float red[PARAMS ? 2 * kBnWaves : 1];
    const bool vg = a.vec & kBnVecG, vy = a.vec & kBnVecYin, vx = a.vec & kBnVecX, vgx = a.vec & kBnVecGx, vgr = a.vec & kBnVecGr;
    const bool want_x = a.gx != nullptr, want_r = a.gr != nullptr;
    for (int q = blockIdx.x; q < a.chunks; q += gridDim.x) {
        const BnSpan s = bn_span(a, q);
        const BnChannel ch = bn_channel(a, s.c);
        const int t = threadIdx.x;
        float sb = 0.0f, sw = 0.0f;
        if (t < s.head) {
            const int e = s.f0 + t;
            const float gm = bn_bwd_one<RELU, PARAMS>(ch, a.g[e], RELU ? a.y_in[e] : 0.0f, PARAMS ? a.x[e] : 0.0f, sb, sw);
            if (want_r) a.gr[e] = gm;
            if (want_x) a.gx[e] = gm * ch.k;
        }
        const int body = s.f0 + s.head;
        float4 g[kBnRounds], y[kBnRounds], x[kBnRounds];           // as in the forward: every load before the first use
#pragma unroll
        for (int j = 0; j < kBnRounds; ++j)
            if (j * kBnThreads < s.groups) {
                const int e = body + 4 * min(t + j * kBnThreads, s.groups - 1);
                g[j] = bn_load4(a.g + e, vg);
                if (RELU) y[j] = bn_load4(a.y_in + e, vy);
                if (PARAMS) x[j] = bn_load4(a.x + e, vx);
            }
#pragma unroll
        for (int j = 0; j < kBnRounds; ++j) {
            const int v = t + j * kBnThreads;
            if (v < s.groups) {
                const int e = body + 4 * v;
                float4 m;
                m.x = bn_bwd_one<RELU, PARAMS>(ch, g[j].x, RELU ? y[j].x : 0.0f, PARAMS ? x[j].x : 0.0f, sb, sw);
                m.y = bn_bwd_one<RELU, PARAMS>(ch, g[j].y, RELU ? y[j].y : 0.0f, PARAMS ? x[j].y : 0.0f, sb, sw);
                m.z = bn_bwd_one<RELU, PARAMS>(ch, g[j].z, RELU ? y[j].z : 0.0f, PARAMS ? x[j].z : 0.0f, sb, sw);
                m.w = bn_bwd_one<RELU, PARAMS>(ch, g[j].w, RELU ? y[j].w : 0.0f, PARAMS ? x[j].w : 0.0f, sb, sw);
                if (want_r) bn_store4(a.gr + e, vgr, m);
                if (want_x) bn_store4(a.gx + e, vgx, make_float4(m.x * ch.k, m.y * ch.k, m.z * ch.k, m.w * ch.k));
            }
        }
        const int tail = body + 4 * s.groups + t;
        if (tail < s.f0 + s.n) {
            const float gm = bn_bwd_one<RELU, PARAMS>(ch, a.g[tail], RELU ? a.y_in[tail] : 0.0f, PARAMS ? a.x[tail] : 0.0f, sb, sw);
            if (want_r) a.gr[tail] = gm;
            if (want_x) a.gx[tail] = gm * ch.k;
        }
        if (PARAMS) {
            sb = bn_wave_sum(sb);
            sw = bn_wave_sum(sw);
            const int wave = t >> 6;
            if ((t & 63) == 0) { red[wave] = sb; red[kBnWaves + wave] = sw; }
            __syncthreads();
            if (t < 2) {                        // lane 0: the bias sums' partial; lane 1: the weight sums'
                float acc = 0.0f;
#pragma unroll
                for (int w = 0; w < kBnWaves; ++w) acc = acc + red[t * kBnWaves + w];
                a.part[t * a.chunks + q] = acc;
            }
            __syncthreads();                    // `red` is written again by the next chunk
        }
    }
}

// the header's step 3: one wave per channel
__global__ void __launch_bounds__(kBnFinalThreads) bn_act_backward_final_kernel(const BnArgs a) {
#pragma clang fp contract(off)
    const int c = blockIdx.x, t = threadIdx.x, P = a.N * a.chunks_per_plane;
    float sb = 0.0f, sw = 0.0f;
    for (int p = t; p < P; p += kBnFinalThreads) {
        const int n = p / a.chunks_per_plane, k = p - n * a.chunks_per_plane;
        const int q = (n * a.C + c) * a.chunks_per_plane + k;
        sb = sb + a.part[q];
        sw = sw + a.part[a.chunks + q];
    }
    sb = bn_wave_sum(sb);
    sw = bn_wave_sum(sw);
    if (t == 0) {
        if (a.gb) a.gb[c] = sb;
        if (a.gw) a.gw[c] = sw;
    }
}

// ------------------------------------------------------------------------------------------------ the stem
struct StemArgs {
    const float *x, *mean, *var, *weight, *bias;
    float *p;
    int C, H, W, Ho, Wo, tiles_x, tiles_y, tiles;
    float eps;
};

__global__ void __launch_bounds__(kStemThreads) bn_relu_maxpool_forward_kernel(const StemArgs s) {
#pragma clang fp contract(off)
    __shared__ float tile[kStemRows][kStemCols];
    BnArgs a;
    a.mean = s.mean; a.var = s.var; a.weight = s.weight; a.bias = s.bias; a.eps = s.eps;
    const int per_plane = s.tiles_x * s.tiles_y;
    for (int q = blockIdx.x; q < s.tiles; q += gridDim.x) {
        const int plane = q / per_plane, b = q - plane * per_plane, ty = b / s.tiles_x, tx = b - ty * s.tiles_x;
        const BnChannel ch = bn_channel(a, plane % s.C);
        const int oy0 = ty * kStemTileH, ox0 = tx * kStemTileW, iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;
        const float *in = s.x + (long long)plane * (s.H * s.W);
        // stage y on the window, row-major over the lanes; every load is issued before the first is used (a position outside the map or
        // the window loads the plane's first element and stores nothing)
        float v[kStemStage];
#pragma unroll
        for (int j = 0; j < kStemStage; ++j) {
            const int e = threadIdx.x + j * kStemThreads, r = e / kStemCols, c = e - r * kStemCols, iy = iy0 + r, ix = ix0 + c;
            const bool ok = e < kStemRows * kStemCols && iy >= 0 && iy < s.H && ix >= 0 && ix < s.W;
            v[j] = in[ok ? iy * s.W + ix : 0];
        }
#pragma unroll
        for (int j = 0; j < kStemStage; ++j) {
            const int e = threadIdx.x + j * kStemThreads, r = e / kStemCols, c = e - r * kStemCols, iy = iy0 + r, ix = ix0 + c;
            if (e < kStemRows * kStemCols && iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) tile[r][c] = bn_act_one<false, true>(ch, v[j], 0.0f);
        }
        __syncthreads();
        float *out = s.p + (long long)plane * (s.Ho * s.Wo);
        for (int e = threadIdx.x; e < kStemTileH * kStemTileW; e += kStemThreads) {
            const int ry = e / kStemTileW, rx = e - ry * kStemTileW, oy = oy0 + ry, ox = ox0 + rx;
            if (oy >= s.Ho || ox >= s.Wo) continue;
            float m = -__builtin_inff();
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int iy = 2 * oy - 1 + dy, ix = 2 * ox - 1 + dx;
                    if (iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) {
                        const float v = tile[2 * ry + dy][2 * rx + dx];
                        m = (v > m || v != v) ? v : m;
                    }
                }
            out[oy * s.Wo + ox] = m;
        }
        __syncthreads();                        // the tile is staged again
    }
}
