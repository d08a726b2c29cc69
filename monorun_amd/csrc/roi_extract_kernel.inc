// roi_extract_kernel.inc — the multi-level RoI feature extractor (mmdet's SingleRoIExtractor over mmcv's RoIAlign, DESIGN.md section 18;
// included by monorun_pnp.hip inside its anonymous namespace): ONE launch forward and ONE backward for all levels and RoIs.  The bin
// samplers are noc_decode_kernel.inc's (roi_geom, roi_sample_coord, roi_axis_tap, roi_blend, beside roi_align_avg_bin), contraction is off.
constexpr int kRoiMaxLevels = 8;        // MR_ROI_MAX_LEVELS
constexpr int kRoiMaxOut = 32;          // MR_ROI_MAX_OUT: out_h, out_w
constexpr int kRoiThreads = 256;
constexpr int kRoiChunk = 32;           // MR_ROI_CHUNK: channels of one forward workgroup
constexpr int kRoiTaps = 256;           // MR_ROI_TAPS: per-axis entries (bin, sample) of the forward's LDS geometry table
constexpr int kRoiTileH = 8, kRoiTileW = 32;     // MR_ROI_TILE_H, MR_ROI_TILE_W: the backward's map tile, one pixel per thread
constexpr int kRoiBwdChunk = 8;         // MR_ROI_BWD_CHUNK: channels of one backward workgroup (one accumulator each per thread)
constexpr int kRoiWaves = kRoiThreads / 64;
static_assert(kRoiTileH * kRoiTileW == kRoiThreads, "one map pixel per thread");

struct RoiLevel { float *map; int H, W, stride; unsigned first_block; };      // forward: feats[l] (read only); backward: grad_feats[l]
struct RoiExtractArgs {
    RoiLevel lv[kRoiMaxLevels];         // the level table travels in the kernel arguments
    const float *rois;                  // (K, 5) image, x1, y1, x2, y2
    const float *level_rois;            // (K, 5): the boxes the level rule reads (mmdet rescales the RoIs after it); never NULL here
    float *out;                         // forward: (K, C, oh, ow), written; backward: grad_out, read
    int L, N, C, K, oh, ow, sampling_ratio, aligned;
    float finest_scale;
};

// One RoI's record: its level (the count of i in 1 .. L-1 with v >= 2^i, v = sqrtf(w h) / finest_scale + 1e-6f; a NaN v compares false:
// level 0), its image, its geometry on that level's map.  false for a degenerate RoI (zeros out, no gradient): a coordinate or image
// index that is not finite, an image outside [0, N), or at sampling_ratio 0 a sample grid beyond the map's size + 2 (compared in float,
// before any conversion to int: the sample loops stay bounded whatever the RoI holds).
struct RoiRecord { int level, image; RoiGeom g; };
__device__ __forceinline__ bool roi_record(const RoiExtractArgs &a, int k, RoiRecord &r) {
#pragma clang fp contract(off)
    const float *p = a.rois + (long long)k * 5;
    const float bi = p[0], x1 = p[1], y1 = p[2], x2 = p[3], y2 = p[4];
    const float inf = __int_as_float(0x7f800000);
    if (!(fabsf(bi) < inf && fabsf(x1) < inf && fabsf(y1) < inf && fabsf(x2) < inf && fabsf(y2) < inf)) return false;
    if (!(bi > -1.0f && bi < (float)a.N)) return false;
    r.image = (int)bi;
    const float *q = a.level_rois + (long long)k * 5;
    const float v = sqrtf((q[3] - q[1]) * (q[4] - q[2])) / a.finest_scale + 1e-6f;
    int level = 0;
    float pw2 = 2.0f;
    for (int i = 1; i < a.L; ++i, pw2 = pw2 * 2.0f) level += v >= pw2 ? 1 : 0;
    r.level = level;
    const float scale = 1.0f / (float)a.lv[level].stride;
    if (a.sampling_ratio <= 0) {        // roi_geom's grid, in float: (int)ceilf of a huge or infinite quotient is not defined
        const float off = a.aligned ? 0.5f : 0.0f;
        float rw = (x2 * scale - off) - (x1 * scale - off), rh = (y2 * scale - off) - (y1 * scale - off);
        if (!a.aligned) { rw = fmaxf(rw, 1.0f); rh = fmaxf(rh, 1.0f); }
        if (ceilf(rh / (float)a.oh) > (float)(a.lv[level].H + 2) || ceilf(rw / (float)a.ow) > (float)(a.lv[level].W + 2)) return false;
    }
    r.g = roi_geom(x1 * scale, y1 * scale, x2 * scale, y2 * scale, a.oh, a.ow, a.sampling_ratio, a.aligned);
    return true;
}

// ------------------------------------------------------------------------------------------------ forward
// One workgroup per (RoI, chunk of kRoiChunk channels).  The RoI's sample geometry is separable: per axis one tap record per (bin, sample)
// — the two rows / columns, their weights, dead or not —, computed ONCE per workgroup into LDS (oh gh + ow gw records) and read by every
// channel; a RoI whose table would not fit kRoiTaps records on an axis computes that axis' taps in place (the same routine).  The block of
// outputs of a workgroup, (channels of the chunk) x oh x ow, is contiguous in `out`: thread t takes elements t, t + 256, ...: coalesced
// stores.  Per element the sum is roi_align_avg_bin's: iy outer, ix inner, a dead sample adds 0.0f, one division by count.
struct RoiTapLds { int lo, hi; float l, h; };      // lo < 0: dead
__global__ void __launch_bounds__(kRoiThreads) roi_extract_forward_kernel(const RoiExtractArgs a) {
#pragma clang fp contract(off)
    __shared__ RoiTapLds taps[2][kRoiTaps];
    const int chunks = (a.C + kRoiChunk - 1) / kRoiChunk;
    const int k = blockIdx.x / chunks, c0 = (blockIdx.x - k * chunks) * kRoiChunk;
    const int nc = min(kRoiChunk, a.C - c0), bins = a.oh * a.ow;
    float *out = a.out + ((long long)k * a.C + c0) * bins;
    RoiRecord r;
    if (!roi_record(a, k, r)) {         // the same answer in every thread: the branch is uniform
        for (int e = threadIdx.x; e < nc * bins; e += kRoiThreads) out[e] = 0.0f;
        return;
    }
    const RoiLevel lv = a.lv[__builtin_amdgcn_readfirstlane(r.level)];
    const RoiGeom g = r.g;
    const bool ylds = g.gh > 0 && g.gh <= kRoiTaps / a.oh, xlds = g.gw > 0 && g.gw <= kRoiTaps / a.ow;
    if (ylds)
        for (int e = threadIdx.x; e < a.oh * g.gh; e += kRoiThreads) {
            const int ph = e / g.gh, iy = e - ph * g.gh;
            RoiTap t = { 0, 0, 0.0f, 0.0f };
            const bool dead = roi_axis_tap(roi_sample_coord(g.sh, g.bh, ph, iy, g.gh), lv.H, t);
            taps[0][e] = RoiTapLds{ dead ? -1 : t.lo, t.hi, t.l, t.h };
        }
    if (xlds)
        for (int e = threadIdx.x; e < a.ow * g.gw; e += kRoiThreads) {
            const int pw = e / g.gw, ix = e - pw * g.gw;
            RoiTap t = { 0, 0, 0.0f, 0.0f };
            const bool dead = roi_axis_tap(roi_sample_coord(g.sw, g.bw, pw, ix, g.gw), lv.W, t);
            taps[1][e] = RoiTapLds{ dead ? -1 : t.lo, t.hi, t.l, t.h };
        }
    __syncthreads();
    const float *slab = lv.map + ((long long)r.image * a.C + c0) * lv.H * lv.W;
    const int hw = lv.H * lv.W;
    for (int e = threadIdx.x; e < nc * bins; e += kRoiThreads) {
        const int c = e / bins, bin = e - c * bins, ph = bin / a.ow, pw = bin - ph * a.ow;
        const float *in = slab + c * hw;
        float acc = 0.0f;
        for (int iy = 0; iy < g.gh; ++iy) {
            RoiTap ty;
            bool dead_y;
            if (ylds) { const RoiTapLds s = taps[0][ph * g.gh + iy]; dead_y = s.lo < 0; ty = RoiTap{ s.lo, s.hi, s.l, s.h }; }
            else dead_y = roi_axis_tap(roi_sample_coord(g.sh, g.bh, ph, iy, g.gh), lv.H, ty);
            for (int ix = 0; ix < g.gw; ++ix) {
                RoiTap tx;
                bool dead_x;
                if (xlds) { const RoiTapLds s = taps[1][pw * g.gw + ix]; dead_x = s.lo < 0; tx = RoiTap{ s.lo, s.hi, s.l, s.h }; }
                else dead_x = roi_axis_tap(roi_sample_coord(g.sw, g.bw, pw, ix, g.gw), lv.W, tx);
                float v = 0.0f;
                if (!(dead_y | dead_x)) v = roi_blend(in, lv.W, ty, tx);
                acc += v;
            }
        }
        out[e] = acc / g.count;
    }
}

// ------------------------------------------------------------------------------------------------ backward
// A gather: one workgroup per (level, image, kRoiTileH x kRoiTileW map tile, chunk of kRoiBwdChunk channels), one map pixel per thread,
// one accumulator per channel of the chunk; every element of every grad_feats[l] is stored exactly once (zeros where no RoI reaches).
//   1. The K RoI records are examined in rounds of 256, one per thread: on this level and image, not degenerate, and its tap footprint
//      (the rows / columns its samples can touch, padded) meets the tile.  An ordered ballot + prefix popcount compacts the round's hits
//      into an LDS list, so RoIs are taken in index order whatever the round size.
//   2. Per listed RoI the bilinear weight of a sample is separable, (h or l of its row) x (h or l of its column), and so is the dead rule:
//      Wy[row][ph] = the sum over the bin's samples iy (not dead in y) of the weight the sample gives to that map row, Wx[col][pw] alike,
//      computed cooperatively into LDS by looping over ALL ph and iy through the forward's tap routine (clamped rows included) — no index
//      range is derived, so it cannot disagree with the forward.  The RoI's grad_out block for the chunk is staged in LDS, channel fastest.
//   3. Each thread adds  (sum over ph, pw of (Wy[row][ph] Wx[col][pw]) grad_out[k, c, ph, pw]) / count  per channel, in the order (RoI, ph,
//      pw), skipping zero weights.  No atomics, no memset: bitwise reproducible.
struct RoiBwdLds {
    float wy[kRoiTileH][kRoiMaxOut];
    float wx[kRoiMaxOut][kRoiTileW];             // [pw][column]: the 32 lanes of a tile row read 32 consecutive banks
    float go[kRoiMaxOut * kRoiMaxOut][kRoiBwdChunk];
    int list[kRoiThreads];
    int wave_hits[kRoiWaves];
};
__global__ void __launch_bounds__(kRoiThreads) roi_extract_backward_kernel(const RoiExtractArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) RoiBwdLds s;
    int level = 0;
    for (int l = 1; l < a.L; ++l) level += blockIdx.x >= a.lv[l].first_block ? 1 : 0;
    const RoiLevel lv = a.lv[level];
    const int tiles_x = (lv.W + kRoiTileW - 1) / kRoiTileW, tiles_y = (lv.H + kRoiTileH - 1) / kRoiTileH;
    const int chunks = (a.C + kRoiBwdChunk - 1) / kRoiBwdChunk;
    int b = (int)(blockIdx.x - lv.first_block);
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y; b /= tiles_y;
    const int chunk = b % chunks, image = b / chunks;
    const int c0 = chunk * kRoiBwdChunk, nc = min(kRoiBwdChunk, a.C - c0);
    const int row0 = ty * kRoiTileH, col0 = tx * kRoiTileW;
    const int trow = threadIdx.x / kRoiTileW, tcol = threadIdx.x % kRoiTileW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bins = a.oh * a.ow;
    float acc[kRoiBwdChunk];
#pragma unroll
    for (int j = 0; j < kRoiBwdChunk; ++j) acc[j] = 0.0f;

    for (int k0 = 0; k0 < a.K; k0 += kRoiThreads) {
        // 1. this round's RoIs that reach the tile, compacted in index order
        bool hit = false;
        const int k = k0 + (int)threadIdx.x;
        if (k < a.K) {
            RoiRecord r;
            if (roi_record(a, k, r) && r.level == level && r.image == image && r.g.gh > 0 && r.g.gw > 0) {
                // samples lie between the RoI's two edges; their taps one row further; the pad also covers the rounding of the
                // sample coordinates (a few ulps of the larger edge).  Too wide only costs time: step 2 computes the exact weights.
                const float ya = r.g.sh, yb = r.g.sh + r.g.rh, xa = r.g.sw, xb = r.g.sw + r.g.rw;
                const float pad_y = 2.0f + (fabsf(ya) + fabsf(yb)) * 0x1p-18f, pad_x = 2.0f + (fabsf(xa) + fabsf(xb)) * 0x1p-18f;
                const float ylo = fminf(ya, yb) - pad_y, yhi = fmaxf(ya, yb) + pad_y, xlo = fminf(xa, xb) - pad_x, xhi = fmaxf(xa, xb) + pad_x;
                // a sample beyond the map is clamped onto the last row / column: a tile at the border is met from outside too
                const bool last_y = row0 + kRoiTileH >= lv.H, last_x = col0 + kRoiTileW >= lv.W;
                hit = yhi >= (float)row0 && (last_y || ylo <= (float)(row0 + kRoiTileH - 1)) &&
                      xhi >= (float)col0 && (last_x || xlo <= (float)(col0 + kRoiTileW - 1));
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) s.wave_hits[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kRoiWaves; ++w) { const int n = s.wave_hits[w]; before += w < wave ? n : 0; total += n; }
        if (hit) s.list[before + __popcll(mask & ((1ull << lane) - 1ull))] = k;
        __syncthreads();

        for (int i = 0; i < total; ++i) {
            const int kk = s.list[i];
            RoiRecord r;
            roi_record(a, kk, r);               // listed: not degenerate
            const RoiGeom g = r.g;
            // 2. the separable weights of this RoI on the tile's rows and columns, and its grad_out block
            for (int e = threadIdx.x; e < (kRoiTileH + kRoiTileW) * kRoiMaxOut; e += kRoiThreads) {
                const bool isy = e < kRoiTileH * kRoiMaxOut;
                const int q = isy ? e : e - kRoiTileH * kRoiMaxOut;
                const int line = isy ? q / kRoiMaxOut : q % kRoiTileW, p = isy ? q % kRoiMaxOut : q / kRoiTileW;     // x: lanes along the column, as wx is stored
                const int np = isy ? a.oh : a.ow;
                if (p >= np) continue;
                const int target = (isy ? row0 : col0) + line, size = isy ? lv.H : lv.W, gn = isy ? g.gh : g.gw;
                const float start = isy ? g.sh : g.sw, bin = isy ? g.bh : g.bw;
                float w = 0.0f;
                for (int it = 0; it < gn; ++it) {
                    RoiTap t;
                    if (roi_axis_tap(roi_sample_coord(start, bin, p, it, gn), size, t)) continue;
                    if (t.lo == target) w += t.h;
                    if (t.hi == target) w += t.l;
                }
                if (isy) s.wy[line][p] = w; else s.wx[p][line] = w;
            }
            const float *go = a.out + ((long long)kk * a.C + c0) * bins;
            for (int e = threadIdx.x; e < nc * bins; e += kRoiThreads) {
                const int c = e / bins, bin = e - c * bins;
                s.go[bin][c] = go[e];
            }
            __syncthreads();
            // 3. this pixel's share
            float part[kRoiBwdChunk];
#pragma unroll
            for (int j = 0; j < kRoiBwdChunk; ++j) part[j] = 0.0f;
            for (int ph = 0; ph < a.oh; ++ph) {
                const float wy = s.wy[trow][ph];
                if (wy == 0.0f) continue;
                for (int pw = 0; pw < a.ow; ++pw) {
                    const float w = wy * s.wx[pw][tcol];
                    if (w == 0.0f) continue;
                    const float4 *gp = (const float4 *)s.go[ph * a.ow + pw];
                    const float4 g0 = gp[0], g1 = gp[1];
                    part[0] += w * g0.x; part[1] += w * g0.y; part[2] += w * g0.z; part[3] += w * g0.w;
                    part[4] += w * g1.x; part[5] += w * g1.y; part[6] += w * g1.z; part[7] += w * g1.w;
                }
            }
#pragma unroll
            for (int j = 0; j < kRoiBwdChunk; ++j) acc[j] += part[j] / g.count;
            __syncthreads();                    // the weights and the block are rewritten for the next RoI
        }
    }
    const int row = row0 + trow, col = col0 + tcol;
    if (row < lv.H && col < lv.W) {
        float *dst = lv.map + ((long long)image * a.C + c0) * lv.H * lv.W + row * lv.W + col;
#pragma unroll
        for (int j = 0; j < kRoiBwdChunk; ++j)
            if (j < nc) dst[j * lv.H * lv.W] = acc[j];
    }
}
