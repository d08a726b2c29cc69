// proposals_kernel.inc — the proposal stage (mmdet's RPNHead.get_bboxes and mmcv's nms / batched_nms, DESIGN.md section 19; included by
// monorun_pnp.hip inside its anonymous namespace): the fused proposal decode, ONE launch for every image and level, and the grouped
// axis-aligned NMS, a bit-matrix launch and a scan launch.  Contraction is off: every operation is an fp32 one, as include/monorun_proposals.h
// states them.
constexpr int kPropMaxLevels = 8;       // MR_PROPOSAL_MAX_LEVELS
constexpr int kPropMaxAnchors = 16;     // MR_PROPOSAL_MAX_ANCHORS
constexpr int kPropThreads = 256;
constexpr int kNmsMaxGroup = 4096;      // MR_NMS_MAX_GROUP: 64 lanes x 64 bits
constexpr int kNmsMaxGroups = 65535;    // MR_NMS_MAX_GROUPS: gridDim.y
constexpr int kNmsTile = 64;            // MR_NMS_TILE
constexpr int kNmsScanRows = 32;        // MR_NMS_SCAN_ROWS: rows per register buffer of the scan

// ------------------------------------------------------------------------------------------------ decode
struct ProposalLevel {
    const float *cls, *reg;             // (N, A, H, W), (N, 4A, H, W): the head's outputs as they are
    int H, W, stride;
    int count, first;                   // candidates per image of this level, and of the levels before it
    float base[kPropMaxAnchors][4];
};
struct ProposalArgs {
    ProposalLevel lv[kPropMaxLevels];   // the level table travels in the kernel arguments
    const long long *index;             // (N, per_image) flat anchor indices (y W + x) A + a, level by level in rank order
    const float *img_shape;             // (N, 2) img_h, img_w
    float mean[4], std[4];
    float max_ratio, min_size;
    int L, N, A, per_image;
    float *boxes, *score, *logit;
    uint8_t *valid;
};

// mmdet's delta2bbox of one box and its clamp to the image, the ONE copy every kernel that moves a box by deltas calls (this file's decode,
// bbox_head_kernel.inc's rank launch, roi_train_kernel.inc): d = delta std + mean, dw and dh clamped to +-max_ratio, the centre moved by
// pw dx, the size scaled by expf(dw), the corners clamped to [0, img_w] x [0, img_h].  Every operation is an fp32 one in this order.
__device__ __forceinline__ void delta2bbox_clamped(float bx1, float by1, float bx2, float by2, float d0, float d1, float d2, float d3,
                                                   const float *mean, const float *std, float max_ratio, float img_h, float img_w,
                                                   float &x1, float &y1, float &x2, float &y2) {
#pragma clang fp contract(off)
    const float dx = d0 * std[0] + mean[0], dy = d1 * std[1] + mean[1];
    float dw = d2 * std[2] + mean[2], dh = d3 * std[3] + mean[3];
    dw = fminf(fmaxf(dw, -max_ratio), max_ratio);
    dh = fminf(fmaxf(dh, -max_ratio), max_ratio);
    const float px = (bx1 + bx2) * 0.5f, py = (by1 + by2) * 0.5f, pw = bx2 - bx1, ph = by2 - by1;
    const float gw = pw * expf(dw), gh = ph * expf(dh);
    const float gx = px + pw * dx, gy = py + ph * dy;
    x1 = fminf(fmaxf(gx - gw * 0.5f, 0.0f), img_w); y1 = fminf(fmaxf(gy - gh * 0.5f, 0.0f), img_h);
    x2 = fminf(fmaxf(gx + gw * 0.5f, 0.0f), img_w); y2 = fminf(fmaxf(gy + gh * 0.5f, 0.0f), img_h);
}

// One thread per candidate; blockIdx.y = image * L + level, so the level's row of the table is read with a uniform index.
__global__ void __launch_bounds__(kPropThreads) proposal_decode_kernel(const ProposalArgs a) {
#pragma clang fp contract(off)
    const int n = blockIdx.y / a.L, l = blockIdx.y - n * a.L;
    const ProposalLevel &lv = a.lv[l];
    const int r = blockIdx.x * kPropThreads + threadIdx.x;
    if (r >= lv.count) return;
    const long long pos = (long long)n * a.per_image + lv.first + r;
    const long long t = a.index[pos];
    const int hw = lv.H * lv.W;
    if ((unsigned long long)t >= (unsigned long long)((long long)hw * a.A)) {       // not an anchor of this level: nothing is read
        const float nan = __int_as_float(0x7fc00000);
        for (int c = 0; c < 4; ++c) a.boxes[pos * 4 + c] = nan;
        a.score[pos] = nan; a.logit[pos] = nan; a.valid[pos] = 0;
        return;
    }
    const int cell = (int)(t / a.A), an = (int)(t - (long long)cell * a.A);
    const int y = cell / lv.W, x = cell - y * lv.W;
    const float logit = lv.cls[((long long)n * a.A + an) * hw + cell];
    const float *rg = lv.reg + ((long long)n * 4 * a.A + 4 * an) * hw + cell;
    const float sx = (float)x * (float)lv.stride, sy = (float)y * (float)lv.stride;
    const float ax1 = lv.base[an][0] + sx, ay1 = lv.base[an][1] + sy, ax2 = lv.base[an][2] + sx, ay2 = lv.base[an][3] + sy;
    float x1, y1, x2, y2;
    delta2bbox_clamped(ax1, ay1, ax2, ay2, rg[0], rg[hw], rg[2 * (long long)hw], rg[3 * (long long)hw], a.mean, a.std, a.max_ratio,
                       a.img_shape[2 * n], a.img_shape[2 * n + 1], x1, y1, x2, y2);
    a.boxes[pos * 4 + 0] = x1; a.boxes[pos * 4 + 1] = y1; a.boxes[pos * 4 + 2] = x2; a.boxes[pos * 4 + 3] = y2;
    a.score[pos] = 1.0f / (1.0f + expf(-logit));
    a.logit[pos] = logit;
    a.valid[pos] = (a.min_size > 0.0f && (x2 - x1 < a.min_size || y2 - y1 < a.min_size)) ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ grouped NMS
// The size of group g as both kernels read it: offsets' difference, cut to [0, max_group].
__device__ __forceinline__ int nms_group_size(const int *offsets, int g, int max_group) {
    return min(max(offsets[g + 1] - offsets[g], 0), max_group);
}

// The first 64-bit word of group g's rows in the workspace: sum over the groups before it of n ceil(n / 64), added across the wave's
// lanes (integers: any order gives the same sum).
__device__ __forceinline__ long long nms_group_words(const int *offsets, int g, int max_group, int lane) {
    long long s = 0;
    for (int q = lane; q < g; q += 64) {
        const int n = nms_group_size(offsets, q, max_group);
        s += (long long)n * ((n + kNmsTile - 1) / kNmsTile);
    }
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)s);      // every lane holds the sum: make that known
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)s >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// One wave per 64 x 64 tile (rb, cb), cb >= rb, of a group's suppression matrix: blockIdx.x numbers the tiles of the upper triangle of a
// max_group matrix row by row, blockIdx.y is the group; tiles beyond the group's own size leave at once.  Lane r holds box rb 64 + r and
// writes word cb of its row: bit q set iff box cb 64 + q comes after it and iou > thr.  The 64 column boxes are staged in LDS and read as
// broadcasts.  Row i of a group of n boxes has ceil(n / 64) words, of which words >= i / 64 are written: the scan reads no others.
__global__ void __launch_bounds__(kNmsTile) nms_mask_kernel(const float *boxes, const int *offsets, int max_group, float thr,
                                                            unsigned long long *ws) {
#pragma clang fp contract(off)
    __shared__ float col[kNmsTile][4];
    const int g = blockIdx.y, lane = threadIdx.x;
    const int n = nms_group_size(offsets, g, max_group), c = (n + kNmsTile - 1) / kNmsTile;
    const int nb = (max_group + kNmsTile - 1) / kNmsTile;
    int t = blockIdx.x, rb = 0;
    while (rb < nb && t >= nb - rb) { t -= nb - rb; ++rb; }
    const int cb = rb + t;
    if (cb >= c) return;                // uniform; rb <= cb < c
    const long long first = offsets[g];
    const long long words = nms_group_words(offsets, g, max_group, lane);
    const int i = rb * kNmsTile + lane, j0 = cb * kNmsTile, j = j0 + lane;
    for (int k = 0; k < 4; ++k) col[lane][k] = j < n ? boxes[(first + j) * 4 + k] : 0.0f;
    __syncthreads();
    if (i >= n) return;
    const float *p = boxes + (first + i) * 4;
    const float ax1 = p[0], ay1 = p[1], ax2 = p[2], ay2 = p[3];
    const float area_a = (ax2 - ax1) * (ay2 - ay1);
    const int jn = min(kNmsTile, n - j0);
    unsigned long long bits = 0;
    for (int q = 0; q < jn; ++q) {
        const float bx1 = col[q][0], by1 = col[q][1], bx2 = col[q][2], by2 = col[q][3];
        const float iw = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f), ih = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
        const float inter = iw * ih;
        const float area_b = (bx2 - bx1) * (by2 - by1);
        const float iou = inter / ((area_a + area_b) - inter);
        if (j0 + q > i && iou > thr) bits |= 1ull << q;
    }
    ws[words + (long long)i * c + cb] = bits;
}

__device__ __forceinline__ unsigned long long nms_readlane64(unsigned long long v, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// Rows i0 .. i0 + 31 of a group's matrix into registers: lane w takes word w of each row.  Every load is issued at once, none under a
// branch and none followed by a use: a row past the group reads the last row and a lane outside [wd, c) the nearest word inside it — inside
// the workspace, but words nobody wrote —, and nms_scan_rows drops what they hold.  The row's address is wave-uniform and depends on no
// decision.  c >= 1.
__device__ __forceinline__ void nms_load_rows(unsigned long long (&R)[kNmsScanRows], const unsigned long long *rows, int i0, int n, int c,
                                              int wd, int lane) {
    const int word = min(max(lane, wd), c - 1);
#pragma unroll
    for (int k = 0; k < kNmsScanRows; ++k) R[k] = rows[(unsigned)(min(i0 + k, n - 1) * c + word)];     // < 4096 * 64: 32-bit offsets
}

// The serial part, 32 decisions: `cur` is word `wd` of the removed set, wave-uniform, bit `bit0 + k` of it box k's; a box whose bit is
// clear is kept and ORs its row into the removed set (the lanes in [wd, c) only: `mine`), lane `wd`'s word of it into `cur`.  A row past
// the group has its bit set from the start, so what was loaded for it is never read.  No load depends on a decision.
__device__ __forceinline__ void nms_scan_rows(const unsigned long long (&R)[kNmsScanRows], unsigned long long &cur,
                                              unsigned long long &removed, int wd, int bit0, unsigned long long mine) {
#pragma unroll
    for (int k = 0; k < kNmsScanRows; ++k)
        if (!((cur >> (bit0 + k)) & 1ull)) {
            cur |= nms_readlane64(R[k], wd);
            removed |= R[k] & mine;
        }
}

// One wave per group.  Lane w holds word w of the removed set: at first the boxes that are not valid and the bits past the group, then
// what the kept boxes suppress.  The matrix has bits only for j > i, so bit i never changes after box i's turn: the final set is the
// complement of the kept boxes.  Rows travel through two register buffers of 32: while one is scanned the next 32 rows are in flight.
__global__ void __launch_bounds__(64) nms_scan_kernel(const unsigned long long *ws, const uint8_t *valid, const int *offsets, int max_group,
                                                      uint8_t *keep, int *num_keep) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int n = nms_group_size(offsets, g, max_group), c = (n + kNmsTile - 1) / kNmsTile;
    const long long first = offsets[g];
    const unsigned long long *rows = ws + nms_group_words(offsets, g, max_group, lane);
    unsigned long long removed = 0;
    if (valid) {
        const uint8_t *flags = valid + first;
        for (int w0 = 0; w0 < c; w0 += 8) {     // eight words' flags in flight at a time (a box past the group reads the last box's)
            unsigned ok[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) ok[u] = flags[min((w0 + u) * kNmsTile + lane, n - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned long long b = __ballot((w0 + u) * kNmsTile + lane >= n || ok[u] == 0);
                if (lane == w0 + u) removed = b;
            }
        }
    } else if (lane < c) {
        const int past = n - lane * kNmsTile;   // >= 1: the bits of this word inside the group
        removed = past >= kNmsTile ? 0ull : ~0ull << past;
    }
    unsigned long long A[kNmsScanRows], B[kNmsScanRows];
    if (c > 0) nms_load_rows(A, rows, 0, n, c, 0, lane);
    for (int wd = 0; wd < c; ++wd) {
        nms_load_rows(B, rows, wd * kNmsTile + kNmsScanRows, n, c, wd, lane);
        unsigned long long cur = nms_readlane64(removed, wd);
        const unsigned long long mine = (lane >= wd && lane < c) ? ~0ull : 0ull;
        nms_scan_rows(A, cur, removed, wd, 0, mine);
        if (wd + 1 < c) nms_load_rows(A, rows, (wd + 1) * kNmsTile, n, c, wd + 1, lane);
        nms_scan_rows(B, cur, removed, wd, kNmsScanRows, mine);
    }
    int count = 0;
    for (int w = 0; w < c; ++w) {
        const unsigned long long word = nms_readlane64(removed, w);
        const int i = w * kNmsTile + lane;
        if (i < n) keep[first + i] = (uint8_t)(((word >> lane) & 1ull) ^ 1ull);
        count += __popcll(~word);
    }
    const int total = offsets[g + 1] - offsets[g];              // a group cut to max_group: the boxes past it are not kept
    for (int i = n + lane; i < total; i += 64) keep[first + i] = 0;
    if (lane == 0) num_keep[g] = count;
}
