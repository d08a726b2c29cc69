// carafe_kernel.inc — N10, the NOC head trunk's upsampler (DESIGN.md section 17; included by monorun_pnp.hip inside its anonymous namespace after
// noc_decode_kernel.inc, whose mr_expf it uses): CARAFEPack's kernel normaliser and feature reassembly (mmcv.ops.carafe) fused, forward and
// backward.  With features x (N, C, H, W), the content encoder's raw output m (N, G k^2 s^2, H, W), r = (k - 1) / 2, g = c / (C / G) and, for
// an output pixel (ph, pw), its source pixel (ph / s, pw / s) and sub-position sub = (ph % s) s + pw % s:
//   l_t            = m[n, (g k^2 + t) s^2 + sub, ph / s, pw / s]                      t = iy k + ix < k^2        (pixel_shuffle)
//   w_t            = mr_expf(l_t - max_t l) / sum_t mr_expf(l_t - max_t l)            sum in the order of t      (softmax over the taps)
//   out[n,c,ph,pw] = sum_t x[n, c, ph / s + iy - r, pw / s + ix - r] w_t              fma chain in the order of t, taps outside the map are 0
// Tiling: a workgroup of 256 threads takes one RoI, one tile of 16 x 16 source pixels and one chunk of up to 32 channels of one group; it
// stages the chunk's tile with its halo, zero-filled outside the map, in LDS as a 32 x (16 + k - 1)^2 fp32 image with compile-time strides
// (every window read is a ds_read with an immediate offset), and keeps the k^2 weights of a thread's pixel in registers.  No atomics: every
// sum runs in one thread in a fixed order, so a RoI's results do not depend on the batch it is in.
constexpr int kCarafeTile = 16;             // source pixels per tile side
constexpr int kCarafeChunk = 32;            // channels per LDS image
constexpr int kCarafeThreads = 256;
template <int K> constexpr int kCarafeUnroll = K * K <= 9 ? 4 : 1;               // channels of a chunk loop in flight: bounds the window reads in flight, and with them the registers
template <int K> constexpr int kCarafeWaves = K < 7 ? 3 : 2;       // waves per SIMD the register allocator must allow: what the LDS image allows (51200 B at k = 5, 61952 B at k = 7)

struct CarafeArgs {
    const float *x, *m, *go;                // features; raw encoder output; grad of out (N, C, H s, W s), backward only
    float *out;                             // forward
    float *gx, *gm;                         // backward: grad of x, grad of m (m's layout); either may be NULL
    float *wn;                              // backward workspace: the normalised masks (N, G k^2, H s, W s); written when gx is wanted
    int N, C, H, W, G, s, ls;               // ls = log2 s
    int Cg, cpg;                            // channels per group, chunks per group
    int tiles_x, tiles_y;
};

// the tile image of `cn` channels: rows y0 - r .. y0 - r + TS - 1 of src (plane stride `plane`, row stride `rs`, column stride `cs`), zero
// outside [0, H) x [0, W) and, with ZERO_TAIL, for the channels cn .. 31
template <int K, bool ZERO_TAIL>
__device__ __forceinline__ void carafe_stage(float *xs, const float *src, size_t plane, size_t rs, int cs, int cn, int y0, int x0, int H, int W) {
    constexpr int TS = kCarafeTile + K - 1, R = (K - 1) / 2;
    const int total = (ZERO_TAIL ? kCarafeChunk : cn) * TS * TS;
    for (int i = threadIdx.x; i < total; i += kCarafeThreads) {
        const int c = i / (TS * TS), rem = i - c * (TS * TS);
        const int ty = rem / TS, tx = rem - ty * TS;
        const int y = y0 - R + ty, x = x0 - R + tx;
        float v = 0.0f;
        if (c < cn && y >= 0 && y < H && x >= 0 && x < W) v = src[(size_t)c * plane + (size_t)y * rs + (size_t)x * cs];
        xs[i] = v;
    }
}

// the k^2 normalised weights of one output pixel: l points at tap 0's logit, the taps are `stride` elements apart (offsets inside one RoI
// fit 32 bits: the host checks)
template <int K>
__device__ __forceinline__ void carafe_softmax(const float *l, unsigned stride, float (&w)[K * K]) {
    // the tap stride is opaque to the optimiser here: else the k^2 uniform tap offsets are hoisted out of the caller's pixel loop and, at k = 7,
    // the 49 scalar address pairs they make do not fit the scalar registers
    asm volatile("" : "+s"(stride));
    float mx = -__int_as_float(0x7f800000);
#pragma unroll
    for (int t = 0; t < K * K; ++t) { w[t] = l[(unsigned)t * stride]; mx = fmaxf(mx, w[t]); }
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        w[t] = mr_expf(w[t] - mx);
        sum += w[t];
        if (t % K == K - 1) __builtin_amdgcn_sched_barrier(0);                 // a row of exponentials at a time: their temporaries stay few
    }
#pragma unroll
    for (int t = 0; t < K * K; ++t) w[t] = w[t] / sum;
}

// workgroup -> (tile, chunk, RoI), tile fastest
struct CarafeBlock { int n, g, c0, cn, y0, x0, th, tw; };
__device__ __forceinline__ CarafeBlock carafe_block(const CarafeArgs &a, unsigned bid) {
    CarafeBlock b;
    const unsigned ntile = (unsigned)(a.tiles_x * a.tiles_y), nchunk = (unsigned)(a.G * a.cpg);
    const unsigned tile = bid % ntile;
    bid /= ntile;
    const int ck = (int)(bid % nchunk);
    b.n = (int)(bid / nchunk);
    b.g = ck / a.cpg;
    b.c0 = b.g * a.Cg + (ck - b.g * a.cpg) * kCarafeChunk;
    b.cn = min(kCarafeChunk, (b.g + 1) * a.Cg - b.c0);
    const int ty = (int)tile / a.tiles_x, tx = (int)tile - ty * a.tiles_x;
    b.y0 = ty * kCarafeTile; b.x0 = tx * kCarafeTile;
    b.th = min(kCarafeTile, a.H - b.y0); b.tw = min(kCarafeTile, a.W - b.x0);
    return b;
}

// Forward, one launch: threads stride over the tile's th s x tw s output pixels; per pixel the softmax of its k^2 logits, then one fma chain and
// one store per channel of the chunk.  Neighbouring lanes are neighbouring output pixels of a row: their stores coalesce, and s of them read the
// same LDS address (a broadcast).
template <int K>
__global__ void __launch_bounds__(kCarafeThreads, kCarafeWaves<K>) carafe_pack_forward_kernel(const CarafeArgs a) {
    constexpr int TS = kCarafeTile + K - 1;
    __shared__ float xs[kCarafeChunk * TS * TS];
    const CarafeBlock b = carafe_block(a, blockIdx.x);
    const unsigned hw = (unsigned)(a.H * a.W);
    const int s2 = a.s * a.s, WO = a.W << a.ls;
    const unsigned hwo = hw * (unsigned)s2;
    carafe_stage<K, false>(xs, a.x + ((size_t)b.n * a.C + b.c0) * hw, hw, a.W, 1, b.cn, b.y0, b.x0, a.H, a.W);
    __syncthreads();
    const int ow = b.tw << a.ls, npix = (b.th << a.ls) * ow;
    const float *mn = a.m + ((size_t)b.n * a.G + b.g) * (K * K) * s2 * hw;
    float *outn = a.out + ((size_t)b.n * a.C + b.c0) * hwo;
    for (int p = threadIdx.x; p < npix; p += kCarafeThreads) {
        const int py = p / ow, px = p - py * ow;
        const int sy = py >> a.ls, sx = px >> a.ls;
        const int sub = ((py & (a.s - 1)) << a.ls) | (px & (a.s - 1));          // the tile's origin is a multiple of s
        float w[K * K];
        carafe_softmax<K>(mn + ((unsigned)sub * hw + (unsigned)((b.y0 + sy) * a.W + (b.x0 + sx))), (unsigned)s2 * hw, w);
        const float *xp = xs + sy * TS + sx;
        float *op = outn + (unsigned)(((b.y0 << a.ls) + py) * WO + ((b.x0 << a.ls) + px));
#pragma unroll kCarafeUnroll<K>
        for (int c = 0; c < b.cn; ++c) {
            float acc = 0.0f;
#pragma unroll
            for (int t = 0; t < K * K; ++t) acc = fmaf(xp[c * (TS * TS) + (t / K) * TS + (t % K)], w[t], acc);
            op[(unsigned)c * hwo] = acc;
        }
    }
}

// Backward, first launch: grad_m and the normalised masks.  A workgroup takes 256 output pixels of one tile, one group and one RoI, and walks
// ALL the group's channels in chunks, in order, so the channel reduction grad_w_t = sum_c grad_out[c] x[c, window t] is one fma chain per
// thread; then  grad_l_t = w_t (grad_w_t - sum_t w_t grad_w_t)  goes to m's layout (the inverse pixel shuffle) and w_t to the workspace.
// blockIdx.x -> (pixel block < s^2, tile, group, RoI).  Without gm only the masks are written (no channel loop).
template <int K>
__global__ void __launch_bounds__(kCarafeThreads, kCarafeWaves<K>) carafe_pack_backward_mask_kernel(const CarafeArgs a) {
    constexpr int TS = kCarafeTile + K - 1;
    __shared__ float xs[kCarafeChunk * TS * TS];
    const int s2 = a.s * a.s;
    unsigned bid = blockIdx.x;
    const int pb = (int)(bid % (unsigned)s2);
    bid /= (unsigned)s2;
    const unsigned ntile = (unsigned)(a.tiles_x * a.tiles_y);
    const int tile = (int)(bid % ntile);
    bid /= ntile;
    const int g = (int)(bid % (unsigned)a.G), n = (int)(bid / (unsigned)a.G);
    const int tyi = tile / a.tiles_x, txi = tile - tyi * a.tiles_x;
    const int y0 = tyi * kCarafeTile, x0 = txi * kCarafeTile;
    const int th = min(kCarafeTile, a.H - y0), tw = min(kCarafeTile, a.W - x0);
    const int ow = tw << a.ls, npix = (th << a.ls) * ow;
    if (pb * kCarafeThreads >= npix) return;                                    // the whole workgroup: an edge tile has fewer pixel blocks
    const int p = pb * kCarafeThreads + threadIdx.x;
    const bool active = p < npix;
    const int py = active ? p / ow : 0, px = active ? p - py * ow : 0;
    const int sy = py >> a.ls, sx = px >> a.ls;
    const int sub = ((py & (a.s - 1)) << a.ls) | (px & (a.s - 1));
    const unsigned hw = (unsigned)(a.H * a.W), hwo = hw * (unsigned)s2;
    const int WO = a.W << a.ls;
    const unsigned opix = (unsigned)(((y0 << a.ls) + py) * WO + ((x0 << a.ls) + px));
    float gw[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) gw[t] = 0.0f;
    if (a.gm) {
        const float *xp = xs + sy * TS + sx;
        for (int ck = 0; ck < a.cpg; ++ck) {
            const int c0 = g * a.Cg + ck * kCarafeChunk, cn = min(kCarafeChunk, (g + 1) * a.Cg - c0);
            __syncthreads();
            carafe_stage<K, false>(xs, a.x + ((size_t)n * a.C + c0) * hw, hw, a.W, 1, cn, y0, x0, a.H, a.W);
            __syncthreads();
            if (active) {
                const float *gp = a.go + ((size_t)n * a.C + c0) * hwo + opix;
#pragma unroll kCarafeUnroll<K>
                for (int c = 0; c < cn; ++c) {
                    const float gov = gp[(unsigned)c * hwo];
#pragma unroll
                    for (int t = 0; t < K * K; ++t) gw[t] = fmaf(gov, xp[c * (TS * TS) + (t / K) * TS + (t % K)], gw[t]);
                }
            }
        }
    }
    if (!active) return;
    float w[K * K];
    const size_t moff = (((size_t)n * a.G + g) * (K * K) * s2 + sub) * hw + (unsigned)((y0 + sy) * a.W + (x0 + sx));
    carafe_softmax<K>(a.m + moff, (unsigned)s2 * hw, w);
    if (a.wn) {
        float *wp = a.wn + ((size_t)n * a.G + g) * (K * K) * hwo + opix;
#pragma unroll
        for (int t = 0; t < K * K; ++t) wp[(unsigned)t * hwo] = w[t];
    }
    if (a.gm) {
        float dot = 0.0f;
#pragma unroll
        for (int t = 0; t < K * K; ++t) dot = fmaf(w[t], gw[t], dot);
        float *gp = a.gm + moff;
#pragma unroll
        for (int t = 0; t < K * K; ++t) gp[(unsigned)(t * s2) * hw] = w[t] * (gw[t] - dot);
    }
}

// Backward, second launch: grad_x as a GATHER.  grad_x[c, y, x] = sum_sub sum_t grad_out[c, (y - iy + r) s + dy, (x - ix + r) s + dx]
// w_t[(y - iy + r) s + dy, (x - ix + r) s + dx]: per sub-position (dy, dx) the same windowed sum as the forward at source resolution, over
// the neighbours' weights.  A thread per source pixel of the tile; per sub-position the workgroup stages the chunk's grad_out samples of that
// sub-position (with halo) in LDS, the thread loads the k^2 neighbour weights from the workspace into registers and adds one fma chain to each of
// the chunk's 32 accumulators, which stay in registers over the s^2 sub-positions.  Fixed order: sub, then t.
template <int K>
__global__ void __launch_bounds__(kCarafeThreads, kCarafeWaves<K>) carafe_pack_backward_input_kernel(const CarafeArgs a) {
    constexpr int TS = kCarafeTile + K - 1, R = (K - 1) / 2;
    __shared__ float gs[kCarafeChunk * TS * TS];
    const CarafeBlock b = carafe_block(a, blockIdx.x);
    const int ty = threadIdx.x / kCarafeTile, tx = threadIdx.x % kCarafeTile;
    const bool active = ty < b.th && tx < b.tw;
    const int y = b.y0 + ty, x = b.x0 + tx;
    const unsigned hw = (unsigned)(a.H * a.W);
    const int s2 = a.s * a.s, WO = a.W << a.ls;
    const unsigned hwo = hw * (unsigned)s2;
    const float *gon = a.go + ((size_t)b.n * a.C + b.c0) * hwo;
    const float *wnn = a.wn + ((size_t)b.n * a.G + b.g) * (K * K) * hwo;
    float acc[kCarafeChunk];
#pragma unroll
    for (int c = 0; c < kCarafeChunk; ++c) acc[c] = 0.0f;
    for (int sub = 0; sub < s2; ++sub) {
        const int dy = sub >> a.ls, dx = sub & (a.s - 1);
        __syncthreads();
        carafe_stage<K, true>(gs, gon + (size_t)dy * WO + dx, hwo, (size_t)a.s * WO, a.s, b.cn, b.y0, b.x0, a.H, a.W);
        __syncthreads();
        if (!active) continue;
        float w[K * K];
#pragma unroll
        for (int t = 0; t < K * K; ++t) {
            // the source pixel whose tap t reads (y, x), clamped into the map: outside it the staged grad_out is 0, so any finite weight serves
            const int by = min(max(y - t / K + R, 0), a.H - 1), bx = min(max(x - t % K + R, 0), a.W - 1);
            w[t] = wnn[(unsigned)t * hwo + (unsigned)((by * a.s + dy) * WO + (bx * a.s + dx))];
            if (t % K == K - 1) __builtin_amdgcn_sched_barrier(0);             // a row of addresses at a time
        }
        const float *gp = gs + ty * TS + tx;
#pragma unroll
        for (int c = 0; c < kCarafeChunk; ++c) {
#pragma unroll
            for (int t = 0; t < K * K; ++t) acc[c] = fmaf(gp[c * (TS * TS) + (K - 1 - t / K) * TS + (K - 1 - t % K)], w[t], acc[c]);
            if (c % kCarafeUnroll<K> == kCarafeUnroll<K> - 1) __builtin_amdgcn_sched_barrier(0);        // as the other kernels' chunk loops: a bounded number of channels in flight
        }
    }
    if (!active) return;
    float *gxp = a.gx + ((size_t)b.n * a.C + b.c0) * hw + (unsigned)(y * a.W + x);
#pragma unroll
    for (int c = 0; c < kCarafeChunk; ++c)
        if (c < b.cn) gxp[(unsigned)c * hw] = acc[c];
}
