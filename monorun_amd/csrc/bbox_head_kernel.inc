// bbox_head_kernel.inc — the 2-D detection head's get_bboxes (mmdet's Shared2FCBBoxHead.get_bboxes: softmax, delta2bbox per class,
// multiclass_nms; DESIGN.md section 20; included by monorun_pnp.hip inside its anonymous namespace): the launch in front of the grouped NMS
// of proposals_kernel.inc, which scores, ranks and decodes the candidates of every (image, class), and the launch behind it, which takes
// each image's first max_num kept candidates.  Contraction is off: every operation is an fp32 one, as include/monorun_bbox.h states them.
constexpr int kBboxMaxRois = 4096;      // MR_BBOX_MAX_ROIS = MR_NMS_MAX_GROUP: the rows of one image
constexpr int kBboxMaxClasses = 16;     // MR_BBOX_MAX_CLASSES
constexpr int kBboxThreads = 1024;
constexpr int kBboxWords = kBboxMaxRois / 64;       // 64-bit words of one class's kept flags

// The rows of image n as every kernel of the stage reads them: row_offsets cut to [0, R] and made monotone, the count cut to max_rois.
// `first`: the image's first row; K: the rows that take part.
__device__ __forceinline__ void bbox_image_rows(const int *row_offsets, int n, int R, int max_rois, int &first, int &K) {
    first = min(max(row_offsets[n], 0), R);
    K = min(min(max(row_offsets[n + 1], first), R) - first, max_rois);
}

struct BboxRankArgs {
    const float *cls, *reg, *rois;      // (R, C + 1) logits, (R, 4C) or (R, 4) deltas, (R, 5) [image, x1, y1, x2, y2]
    const int *row_offsets;             // (N + 1,)
    const float *img_shape, *scale;     // (N, 2) img_h, img_w; (N, 4) or NULL (no rescale)
    int R, N, C, agnostic, max_rois;
    float mean[4], std[4];
    float max_ratio, score_thr;
    float *boxes, *score;
    int *order;
    uint8_t *valid;
    int *group_offsets;                 // (N C + 1,)
};

// The softmax score of class c of one row: m = max x_j, e_j = expf(x_j - m), s = e_0 + e_1 + ... in index order, e_c / s.
__device__ __forceinline__ float bbox_class_score(const float *x, int C, int c) {
#pragma clang fp contract(off)
    float m = x[0];
    for (int j = 1; j <= C; ++j) m = fmaxf(m, x[j]);
    float s = expf(x[0] - m), ec = s;
    for (int j = 1; j <= C; ++j) {
        const float e = expf(x[j] - m);
        s = s + e;
        if (j == c) ec = e;
    }
    return ec / s;
}

// One workgroup per (class, image): blockIdx.x = c, blockIdx.y = n.  The K rows' keys (score descending, NaN after every number, ties to the
// lower row) are sorted in LDS by a bitonic network on 64-bit words padded to the next power of two — the high word orders the scores, the
// low word is the row, so no two keys are equal and the result does not depend on the network —; then thread p decodes the box of the row
// at rank p and writes it at position p of group (n, c), which starts at C first_n + c K.
__global__ void __launch_bounds__(kBboxThreads) bbox_head_rank_kernel(const BboxRankArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned long long keys[kBboxMaxRois];
    const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    int first, K;
    bbox_image_rows(a.row_offsets, n, a.R, a.max_rois, first, K);
    const long long group = (long long)a.C * first + (long long)c * K;
    if (tid == 0) {
        a.group_offsets[n * a.C + c] = (int)group;
        if (n == a.N - 1 && c == a.C - 1) a.group_offsets[a.N * a.C] = a.C * min(max(a.row_offsets[a.N], first), a.R);
    }
    if (K == 0) return;                 // uniform
    int P = 1;
    while (P < K) P <<= 1;
    for (int i = tid; i < P; i += kBboxThreads) {
        unsigned hi = 0xffffffffu;      // padding: after everything
        if (i < K) {
            const float s = bbox_class_score(a.cls + (long long)(first + i) * (a.C + 1), a.C, c);
            const unsigned u = __float_as_uint(s);
            hi = s != s ? 0xfffffffeu : ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));     // ascending in the key = descending in the score
        }
        keys[i] = ((unsigned long long)hi << 32) | (unsigned)i;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kBboxThreads) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;         // bit j of i is clear; i < l < P
                const unsigned long long x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
            }
            __syncthreads();
        }
    const float nan = __uint_as_float(0x7fc00000u);
    for (int p = tid; p < K; p += kBboxThreads) {
        const unsigned long long key = keys[p];
        const int i = (int)(unsigned)key;
        const unsigned hi = (unsigned)(key >> 32), v = ~hi;
        const float s = hi == 0xfffffffeu ? nan : __uint_as_float((v & 0x80000000u) ? (v & 0x7fffffffu) : ~v);
        const long long row = first + i;
        const float *roi = a.rois + row * 5, *d = a.reg + row * (a.agnostic ? 4 : 4 * a.C) + (a.agnostic ? 0 : 4 * c);
        const float rx1 = roi[1], ry1 = roi[2], rx2 = roi[3], ry2 = roi[4];
        float x1, y1, x2, y2;
        delta2bbox_clamped(rx1, ry1, rx2, ry2, d[0], d[1], d[2], d[3], a.mean, a.std, a.max_ratio, a.img_shape[2 * n], a.img_shape[2 * n + 1],
                           x1, y1, x2, y2);
        if (a.scale) {
            const float *f = a.scale + 4 * n;
            x1 = x1 / f[0]; y1 = y1 / f[1]; x2 = x2 / f[2]; y2 = y2 / f[3];
        }
        const bool finite = fabsf(rx1) < INFINITY && fabsf(ry1) < INFINITY && fabsf(rx2) < INFINITY && fabsf(ry2) < INFINITY;
        float *b = a.boxes + (group + p) * 4;
        b[0] = x1; b[1] = y1; b[2] = x2; b[3] = y2;
        a.score[group + p] = s;
        a.order[group + p] = i;
        a.valid[group + p] = (s > a.score_thr && finite) ? 1 : 0;
    }
}

struct BboxSelectArgs {
    const float *boxes, *score;         // the rank launch's outputs
    const int *order;
    const uint8_t *keep;                // the NMS's flags, in the groups' layout
    const int *row_offsets;
    int R, N, C, max_rois, max_num;
    float *dets;                        // (N, max_num, 5)
    long long *labels;                  // (N, max_num)
    int *counts;                        // (N,)
};

// The kept flags of one class below position q of its list: the words before q's and the bits below q in its own.  q <= K.
__device__ __forceinline__ int bbox_kept_below(const unsigned long long *words, const int *pre, int w0, int Kw, int q) {
    const int w = q >> 6;
    if (w == Kw) return pre[w0 + Kw - 1] + __popcll(words[w0 + Kw - 1]);
    return pre[w0 + w] + __popcll(words[w0 + w] & ((1ull << (q & 63)) - 1ull));
}

// One workgroup per image.  Each class's list is in rank order, which is the selection order (score descending, ties to the lower
// candidate r C + c) restricted to the class; so the output position of a kept candidate is the number of kept candidates before it in its
// own list plus, for every other class, the number of kept candidates of that list that precede it — a binary search for the first entry
// of that list that does not precede it, and a prefix count of the kept flags there.  The flags are packed into 64-bit words in LDS with
// a running count per word.  Every position below the count is written by exactly one thread: no atomics, no second sort.
__global__ void __launch_bounds__(kBboxThreads) bbox_head_select_kernel(const BboxSelectArgs a) {
    __shared__ unsigned long long words[kBboxMaxClasses * kBboxWords];
    __shared__ int pre[kBboxMaxClasses * kBboxWords];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, C = a.C;
    int first, K;
    bbox_image_rows(a.row_offsets, n, a.R, a.max_rois, first, K);
    const long long base = (long long)C * first;
    const int Kw = (K + 63) >> 6, nw = C * Kw;
    for (int W = tid >> 6; W < nw; W += kBboxThreads / 64) {       // uniform per wave
        const int c = W / Kw, p = (W - c * Kw) * 64 + lane;
        const unsigned long long bits = __ballot(p < K && a.keep[base + (long long)c * K + p] != 0);
        if (lane == 0) words[W] = bits;
    }
    __syncthreads();
    for (int W = tid; W < nw; W += kBboxThreads) {
        const int w0 = (W / Kw) * Kw;
        int s = 0;
        for (int w = w0; w < W; ++w) s += __popcll(words[w]);
        pre[W] = s;
    }
    __syncthreads();
    int total = 0;
    if (Kw > 0)
        for (int c = 0; c < C; ++c) total += bbox_kept_below(words, pre, c * Kw, Kw, K);
    const int count = min(total, a.max_num);
    float *dets = a.dets + (long long)n * a.max_num * 5;
    long long *labels = a.labels + (long long)n * a.max_num;
    for (int e = tid; e < nw * 64; e += kBboxThreads) {
        const int c = e / (Kw * 64), p = e - c * Kw * 64;
        if (p >= K || !((words[c * Kw + (p >> 6)] >> (p & 63)) & 1ull)) continue;
        int pos = bbox_kept_below(words, pre, c * Kw, Kw, p);
        if (pos >= a.max_num) continue;
        const long long mine = base + (long long)c * K + p;
        const float s = a.score[mine];
        const long long cand = (long long)a.order[mine] * C + c;
        for (int c2 = 0; c2 < C && pos < a.max_num; ++c2) {
            if (c2 == c) continue;
            const long long other = base + (long long)c2 * K;
            int lo = 0, hi = K;                     // the first entry of list c2 that does not precede the candidate
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const float s2 = a.score[other + mid];
                const bool before = s2 > s || (s2 == s && (long long)a.order[other + mid] * C + c2 < cand);
                if (before) lo = mid + 1; else hi = mid;
            }
            pos += bbox_kept_below(words, pre, c2 * Kw, Kw, lo);
        }
        if (pos >= a.max_num) continue;
        const float *b = a.boxes + mine * 4;
        float *o = dets + (long long)pos * 5;
        o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3]; o[4] = s;
        labels[pos] = c;
    }
    const float nan = __uint_as_float(0x7fc00000u);
    for (int t = count + tid; t < a.max_num; t += kBboxThreads) {
        for (int k = 0; k < 5; ++k) dets[(long long)t * 5 + k] = nan;
        labels[t] = -1;
    }
    if (tid == 0) a.counts[n] = count;
}
