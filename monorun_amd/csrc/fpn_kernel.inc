// fpn_kernel.inc — the feature pyramid's top-down pathway (mmdet's FPN / the reference's FPNplus between the lateral and the output
// convolutions, DESIGN.md section 22; included by monorun_pnp.hip inside its anonymous namespace): ONE launch forward and ONE backward
// for all levels.  include/monorun_fpn.h defines the op; contraction is off, every operation is an fp32 one rounded on its own.
constexpr int kFpnMaxLevels = 6;        // MR_FPN_MAX_LEVELS
constexpr int kFpnThreads = 256;
constexpr int kFpnTileH = 16, kFpnTileW = 64;       // MR_FPN_TILE_H, MR_FPN_TILE_W: the forward's tile of the finest level under `low`
constexpr int kFpnFlat = 1024;          // MR_FPN_FLAT: elements of a forward workgroup on every other level
constexpr int kFpnBwdEven = 6144, kFpnBwdOdd = 1536;        // MR_FPN_BWD_EVEN, MR_FPN_BWD_ODD: floats of the backward's two LDS buffers
constexpr int kFpnBwdRows = 32, kFpnBwdCols = 48;           // MR_FPN_BWD_ROWS, MR_FPN_BWD_COLS: the largest footprint of a level that has children

// forward: in = lat[l], out = merged[l]; backward: in = grad_merged[l] (may be NULL: zeros), out = grad_lat[l] (may be NULL: not stored).
// ry, rx: (float)H[l+1] / (float)H[l], the scale of the nearest rule towards the next coarser level, divided once on the host.
struct FpnLevel { const float *in; float *out; int H, W; float ry, rx; unsigned first_block; };
struct FpnArgs {
    FpnLevel lv[kFpnMaxLevels];         // the level table travels in the kernel arguments
    const float *grad_low;              // backward: (planes, 2 H0, 2 W0) or NULL
    float *low;                         // forward: (planes, 2 H0, 2 W0), written when `lower`
    int L, planes, lower;               // planes = n_images channels; lower: 1 with lower_scale 2
    int low_vec;                        // floats per store of `low`: 4 (W0 even, 16-byte aligned), 2 (8-byte aligned) or 1
    int root_h, root_w;                 // backward: the block of coarsest pixels one workgroup owns
};

// the nearest rule: the pixel of the coarser level (Hp of them along this axis) that pixel y of the finer one reads
__host__ __device__ inline int fpn_idx(int y, float r, int Hp) {
    const int i = (int)floorf((float)y * r);
    return i < Hp - 1 ? i : Hp - 1;
}

// the smallest y in [0, Hc] with fpn_idx(y) >= p (Hc: none).  fpn_idx does not decrease with y, so the children of p are
// [first_child(p), first_child(p + 1)); the quotient is only a first guess, the answer is searched with the forward's own rule.
__host__ __device__ inline int fpn_first_child(int p, float r, int Hc, int Hp) {
    if (p <= 0) return 0;
    const float g = (float)p / r;
    int y = g < (float)Hc ? (int)g : Hc;
    while (y > 0 && fpn_idx(y - 1, r, Hp) >= p) --y;
    while (y < Hc && fpn_idx(y, r, Hp) < p) ++y;
    return y;
}

// m[l+1] at the pixel that (y, x) of level l reads: lat[l+1][p1] + (lat[l+2][p2] + ( ... + lat[L-1][p])), added coarsest first as the
// in-place chain adds.  The coarser levels are a quarter, a sixteenth ... of level l: these loads hit the caches.  l + 1 < L.
__device__ __forceinline__ float fpn_coarser(const FpnArgs &a, int l, long long plane, int y, int x) {
#pragma clang fp contract(off)
    float v[kFpnMaxLevels];
#pragma unroll
    for (int k = 1; k < kFpnMaxLevels; ++k) {
        v[k] = 0.0f;
        if (l + k < a.L) {
            const FpnLevel &f = a.lv[l + k - 1], &c = a.lv[l + k];
            y = fpn_idx(y, f.ry, c.H);
            x = fpn_idx(x, f.rx, c.W);
            v[k] = c.in[plane * (c.H * c.W) + y * c.W + x];
        }
    }
    float acc = 0.0f;
    bool have = false;
#pragma unroll
    for (int k = kFpnMaxLevels - 1; k >= 1; --k)
        if (l + k < a.L) { acc = have ? v[k] + acc : v[k]; have = true; }
    return acc;
}

// one axis of the bilinear x2 rule (align_corners=False, torch's rule for a given scale_factor)
struct FpnTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ FpnTap fpn_tap(int Y, int H) {
#pragma clang fp contract(off)
    const float src = fmaxf(((float)Y + 0.5f) * 0.5f - 0.5f, 0.0f);
    FpnTap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < H - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// ------------------------------------------------------------------------------------------------ forward
// A stream.  Under `low` the finest level is cut into kFpnTileH x kFpnTileW tiles of one (image, channel) plane: the workgroup forms
// m[0] on the tile and a halo of one pixel in LDS (a wave reads and writes one 256-byte tile row per instruction), stores the tile, and
// forms the 2 kFpnTileH x 2 kFpnTileW block of `low` from LDS alone — 16 bytes per lane, 512 contiguous bytes per row, where W0 is even
// and `low` is 16-byte aligned.  Every other level that is written (l < L - 1) is a flat stream of kFpnFlat elements per workgroup.
__global__ void __launch_bounds__(kFpnThreads) fpn_topdown_forward_kernel(const FpnArgs a) {
#pragma clang fp contract(off)
    __shared__ float tile[kFpnTileH + 2][kFpnTileW + 2];
    int level = 0;
    for (int l = 1; l < a.L; ++l) level += blockIdx.x >= a.lv[l].first_block ? 1 : 0;
    const FpnLevel lv = a.lv[level];
    const unsigned b = blockIdx.x - lv.first_block;
    const int H = lv.H, W = lv.W, HW = H * W;
    const bool top = level + 1 < a.L;           // something is added and stored; else m[level] is lat[level] itself
    if (level != 0 || !a.lower) {
        const long long total = (long long)a.planes * HW;
        for (int it = 0; it < kFpnFlat / kFpnThreads; ++it) {
            const long long e = (long long)b * kFpnFlat + it * kFpnThreads + threadIdx.x;
            if (e >= total) break;
            const long long plane = e / HW;
            const int p = (int)(e - plane * HW), y = p / W, x = p - y * W;
            lv.out[e] = lv.in[e] + fpn_coarser(a, level, plane, y, x);
        }
        return;
    }
    const int tiles_x = (W + kFpnTileW - 1) / kFpnTileW, tiles_y = (H + kFpnTileH - 1) / kFpnTileH;
    const int tx = b % tiles_x, ty = (b / tiles_x) % tiles_y;
    const long long plane = b / (tiles_x * tiles_y);
    const int y0 = ty * kFpnTileH, x0 = tx * kFpnTileW;
    const float *in = lv.in + plane * HW;
    float *out = lv.out + plane * HW;           // not dereferenced unless `top`
    // the tile: one row per wave-instruction
    for (int e = threadIdx.x; e < kFpnTileH * kFpnTileW; e += kFpnThreads) {
        const int r = e / kFpnTileW, c = e - r * kFpnTileW, y = y0 + r, x = x0 + c;
        if (y < H && x < W) {
            float v = in[y * W + x];
            if (top) { v = v + fpn_coarser(a, 0, plane, y, x); out[y * W + x] = v; }
            tile[r + 1][c + 1] = v;
        }
    }
    // the halo: the rows above and below (with their corners), the columns left and right; recomputed, not stored
    if (threadIdx.x < 2 * (kFpnTileW + 2) + 2 * kFpnTileH) {
        int r, c;
        if (threadIdx.x < 2 * (kFpnTileW + 2)) { r = threadIdx.x < kFpnTileW + 2 ? 0 : kFpnTileH + 1; c = threadIdx.x % (kFpnTileW + 2); }
        else { const int q = threadIdx.x - 2 * (kFpnTileW + 2); r = 1 + q % kFpnTileH; c = q < kFpnTileH ? 0 : kFpnTileW + 1; }
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            float v = in[y * W + x];
            if (top) v = v + fpn_coarser(a, 0, plane, y, x);
            tile[r][c] = v;
        }
    }
    __syncthreads();
    // low: groups of four columns; every tap lies inside the map, so inside what was staged
    float *low = a.low + plane * 4 * HW;
    const int W2 = 2 * W, H2 = 2 * H;
    for (int e = threadIdx.x; e < 2 * kFpnTileH * (kFpnTileW / 2); e += kFpnThreads) {
        const int Y = 2 * y0 + e / (kFpnTileW / 2), X = 2 * x0 + 4 * (e % (kFpnTileW / 2));
        if (Y >= H2 || X >= W2) continue;
        const FpnTap ty_ = fpn_tap(Y, H);
        const float *r0 = tile[ty_.i0 - y0 + 1], *r1 = tile[ty_.i1 - y0 + 1];
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const FpnTap t = fpn_tap(min(X + j, W2 - 1), W);
            const int c0 = t.i0 - x0 + 1, c1 = t.i1 - x0 + 1;
            o[j] = ty_.l0 * (t.l0 * r0[c0] + t.l1 * r0[c1]) + ty_.l1 * (t.l0 * r1[c0] + t.l1 * r1[c1]);
        }
        float *dst = low + (long long)Y * W2 + X;
        if (a.low_vec == 4) *(float4 *)dst = make_float4(o[0], o[1], o[2], o[3]);           // W2 % 4 == 0: the group is whole
        else if (a.low_vec == 2) {                                                            // W2 is even: each pair is whole
            *(float2 *)dst = make_float2(o[0], o[1]);
            if (X + 2 < W2) *(float2 *)(dst + 2) = make_float2(o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (X + j < W2) dst[j] = o[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// A gather.  One workgroup owns a root_h x root_w block of pixels of the coarsest level of one (image, channel) plane and its FOOTPRINT
// on every level: the pixels whose chain of parents ends in the block.  fpn_idx does not decrease, so a footprint is a rectangle, the
// footprints of the blocks partition every level, and every element is stored exactly once.  The workgroup walks the levels finest first:
//   level 0: G = grad_merged[0] + the transpose of the bilinear rule over grad_low (at most 4 x 4 terms, Y outer, X inner);
//   level l: G = grad_merged[l] + the row-major running sum of the children's G, which the previous step left in LDS;
// stores G to grad_lat[l] and keeps it in LDS (two buffers, alternating) for the next level.  The host has checked that every footprint
// fits its buffer.  The bounds of a footprint and the children of its rows and columns come from fpn_first_child: the forward's rule,
// searched, once per row and column into LDS.
struct FpnBwdLds {
    float even[kFpnBwdEven], odd[kFpnBwdOdd];      // G of the levels 0, 2, 4 and of 1, 3, 5 on the footprint
    int foot[kFpnMaxLevels][4];         // per level the footprint's y0, y1, x0, x1
    int kid_y[kFpnBwdRows + 1], kid_x[kFpnBwdCols + 1];     // the first child row / column of each row / column of the footprint, and the end
};
__global__ void __launch_bounds__(kFpnThreads) fpn_topdown_backward_kernel(const FpnArgs a) {
#pragma clang fp contract(off)
    __shared__ FpnBwdLds s;
    float *const even = s.even, *const odd = s.odd;
    int (*const foot)[4] = s.foot;
    int *const kid_y = s.kid_y, *const kid_x = s.kid_x;
    const FpnLevel &root = a.lv[a.L - 1];
    const int tiles_x = (root.W + a.root_w - 1) / a.root_w, tiles_y = (root.H + a.root_h - 1) / a.root_h;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
    const long long plane = blockIdx.x / (tiles_x * tiles_y);
    if (threadIdx.x < 4) {              // one bound each, from the root's block down the levels
        const bool isy = threadIdx.x < 2, end = threadIdx.x & 1;
        const int step = isy ? a.root_h : a.root_w, size = isy ? root.H : root.W;
        int v = (isy ? ty : tx) * step + (end ? step : 0);
        v = v < size ? v : size;
        foot[a.L - 1][threadIdx.x] = v;
        for (int l = a.L - 2; l >= 0; --l) {
            const FpnLevel &f = a.lv[l], &c = a.lv[l + 1];
            v = fpn_first_child(v, isy ? f.ry : f.rx, isy ? f.H : f.W, isy ? c.H : c.W);
            foot[l][threadIdx.x] = v;
        }
    }
    __syncthreads();
    {   // level 0
        const FpnLevel &f = a.lv[0];
        const int H = f.H, W = f.W, fy0 = foot[0][0], fx0 = foot[0][2], fw = foot[0][3] - fx0, n = (foot[0][1] - fy0) * fw;
        const float *gm = f.in ? f.in + plane * (H * W) : nullptr;
        const float *gl = a.lower && a.grad_low ? a.grad_low + plane * 4 * (H * W) : nullptr;
        float *out = f.out ? f.out + plane * (H * W) : nullptr;
        for (int e = threadIdx.x; e < n; e += kFpnThreads) {
            const int r = e / fw, y = fy0 + r, x = fx0 + (e - r * fw);
            float g = gm ? gm[y * W + x] : 0.0f;
            if (a.lower) {
                float acc = 0.0f;
                if (gl) {
                    // the weights per row and column, 0 outside the map: such a term is a selected +0.0f, which changes no sum — no
                    // branch, and its load stays inside the map
                    const int W2 = 2 * W;
                    float wy[4], wx[4];
                    int ro[4], co[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int Y = 2 * y - 1 + j, X = 2 * x - 1 + j;
                        const float wyj = (j == 0 || j == 3) ? 0.25f : ((j == 1 ? y == 0 : y == H - 1) ? 1.0f : 0.75f);
                        const float wxj = (j == 0 || j == 3) ? 0.25f : ((j == 1 ? x == 0 : x == W - 1) ? 1.0f : 0.75f);
                        const bool oky = Y >= 0 && Y < 2 * H, okx = X >= 0 && X < W2;
                        wy[j] = oky ? wyj : 0.0f; ro[j] = (oky ? Y : 2 * y) * W2;
                        wx[j] = okx ? wxj : 0.0f; co[j] = okx ? X : 2 * x;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float w = wy[j] * wx[i], t = w * gl[ro[j] + co[i]];
                            acc += w != 0.0f ? t : 0.0f;
                        }
                }
                g = g + acc;
            }
            if (out) out[y * W + x] = g;
            even[e] = g;
        }
    }
    for (int l = 1; l < a.L; ++l) {
        __syncthreads();
        const FpnLevel &f = a.lv[l], &ch = a.lv[l - 1];
        const float *kids = (l & 1) ? even : odd;
        float *mine = (l & 1) ? odd : even;
        const int H = f.H, W = f.W, fy0 = foot[l][0], fx0 = foot[l][2], fh = foot[l][1] - fy0, fw = foot[l][3] - fx0, n = fh * fw;
        const int ky0 = foot[l - 1][0], kx0 = foot[l - 1][2], kw = foot[l - 1][3] - kx0;
        if ((int)threadIdx.x <= fh) kid_y[threadIdx.x] = fpn_first_child(fy0 + threadIdx.x, ch.ry, ch.H, H);
        else if (threadIdx.x >= 64 && (int)threadIdx.x - 64 <= fw) kid_x[threadIdx.x - 64] = fpn_first_child(fx0 + threadIdx.x - 64, ch.rx, ch.W, W);
        __syncthreads();
        const float *gm = f.in ? f.in + plane * (H * W) : nullptr;
        float *out = f.out ? f.out + plane * (H * W) : nullptr;
        for (int e = threadIdx.x; e < n; e += kFpnThreads) {
            const int r = e / fw, c = e - r * fw, y = fy0 + r, x = fx0 + c;
            const int cy1 = kid_y[r + 1], cx0 = kid_x[c], cx1 = kid_x[c + 1];
            float s = 0.0f;
            for (int cy = kid_y[r]; cy < cy1; ++cy)
                for (int cx = cx0; cx < cx1; ++cx) s += kids[(cy - ky0) * kw + (cx - kx0)];
            const float g = (gm ? gm[y * W + x] : 0.0f) + s;
            if (out) out[y * W + x] = g;
            mine[e] = g;
        }
    }
}
