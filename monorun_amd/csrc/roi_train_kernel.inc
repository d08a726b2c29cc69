// roi_train_kernel.inc — the hand-over from the 2-D stage to the 3-D heads in MonoRUnRoIHead.forward_train (DESIGN.md section 25; included
// by monorun_pnp.hip inside its anonymous namespace): for every sampled positive of the batch, the RoI moved by its ground-truth class's
// deltas (mmdet's regress_by_class) and everything the 3-D heads take per positive, ONE launch.  Contraction is off: every operation is an
// fp32 one, as include/monorun_roi_train.h states them.
constexpr int kRoiTrainThreads = 64;    // MR_ROI_TRAIN_THREADS: one wave; a few hundred positives spread over as many CUs as they fill

struct RoiTrainArgs {
    const float *bboxes;                // (N, T, 4) the sampler's boxes
    const long long *gt_inds, *labels;  // (N, T)
    const long long *pos_inds;          // (N, num), -1 past an image's count
    const int *pos_offsets;             // (N + 1,) the first positive of each image among the K
    int N, T, num, K;
    const float *reg;                   // (R, 4C) or (R, 4) the bbox head's deltas
    const int *reg_offsets;             // (N,) the row of each image's first positive
    int R, C, agnostic;
    const float *gt3d;                  // (sum G, 7)
    const int *gt_offsets;              // (N + 1,)
    int n_gt, max_gt;                   // the rows of gt3d; the host bound of an image's ground truths
    const float *cam, *img_shape;       // (N, 9), (N, 2) img_h, img_w
    const uint8_t *flip;                // (N,)
    float mean[4], std[4];
    float max_ratio;
    const float *dim_mean, *dim_std;    // (C, 3)
    float *rois, *boxes;                // (K, 5), (K, 4)
    long long *out_labels, *out_gt;     // (K,)
    int *img32;
    long long *img64;
    float *out3d, *out_cam, *out_shape; // (K, 7), (K, 9), (K, 2)
    uint8_t *out_flip;
    float *dim_targets;                 // (K, 3)
};

// One thread per positive k.  Its image n is the last one whose offset is <= k (a search over the N + 1 offsets, which are cut to [0, K]
// and read monotone); j = k - offset is its place in the image's ascending list.  A positive any of whose indices leaves its table — the
// place past `num` or the image's count, the sampled index outside [0, T), the label outside [0, C), the ground truth outside the image's
// first max_gt, the delta row outside [0, R) — is VOID: nothing is read through the index, its floats are 0, its label and ground truth -1.
// Every output element is written by exactly one thread.
__global__ void __launch_bounds__(kRoiTrainThreads) roi_train_positives_kernel(const RoiTrainArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * kRoiTrainThreads + threadIdx.x;
    if (k >= a.K) return;
    int lo = 0, hi = a.N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (min(max(a.pos_offsets[mid], 0), a.K) <= k) lo = mid; else hi = mid - 1;
    }
    const int n = lo;
    const int first = min(max(a.pos_offsets[n], 0), a.K), end = min(max(a.pos_offsets[n + 1], first), a.K);
    const int j = k - first;
    long long t = -1, label = -1, g = -1, row = -1;
    bool live = j >= 0 && j < a.num && k < end;
    if (live) {
        t = a.pos_inds[(long long)n * a.num + j];
        live = t >= 0 && t < a.T;
    }
    if (live) {
        const long long at = (long long)n * a.T + t;
        label = a.labels[at];
        g = a.gt_inds[at] - 1;
        const int g0 = a.gt_offsets[n], G = min(a.gt_offsets[n + 1] - g0, a.max_gt);
        row = (long long)a.reg_offsets[n] + j;
        live = label >= 0 && label < a.C && g >= 0 && g < G && g0 >= 0 && g0 + g < a.n_gt && row >= 0 && row < a.R;
    }
    float x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f, b3[7] = {0, 0, 0, 0, 0, 0, 0}, dt[3] = {0, 0, 0};
    if (live) {
        const float *b = a.bboxes + ((long long)n * a.T + t) * 4;
        const float *d = a.reg + row * (a.agnostic ? 4 : 4 * a.C) + (a.agnostic ? 0 : 4 * label);
        delta2bbox_clamped(b[0], b[1], b[2], b[3], d[0], d[1], d[2], d[3], a.mean, a.std, a.max_ratio, a.img_shape[2 * n], a.img_shape[2 * n + 1],
                           x1, y1, x2, y2);
        const float *s = a.gt3d + ((long long)a.gt_offsets[n] + g) * 7;
        for (int c = 0; c < 7; ++c) b3[c] = s[c];
        for (int c = 0; c < 3; ++c) dt[c] = (b3[c] - a.dim_mean[label * 3 + c]) / a.dim_std[label * 3 + c];
    } else {
        label = -1; g = -1;
    }
    float *r = a.rois + (long long)k * 5, *o = a.boxes + (long long)k * 4;
    r[0] = (float)n; r[1] = x1; r[2] = y1; r[3] = x2; r[4] = y2;
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
    a.out_labels[k] = label;
    a.out_gt[k] = g;
    a.img32[k] = n;
    a.img64[k] = n;
    for (int c = 0; c < 7; ++c) a.out3d[(long long)k * 7 + c] = b3[c];
    for (int c = 0; c < 9; ++c) a.out_cam[(long long)k * 9 + c] = a.cam[n * 9 + c];
    a.out_shape[2 * k] = a.img_shape[2 * n]; a.out_shape[2 * k + 1] = a.img_shape[2 * n + 1];
    a.out_flip[k] = a.flip[n] ? 1 : 0;
    for (int c = 0; c < 3; ++c) a.dim_targets[(long long)k * 3 + c] = dt[c];
}
