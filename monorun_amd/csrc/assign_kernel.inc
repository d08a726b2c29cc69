// assign_kernel.inc — the 2-D detector's target assignment (mmdet's MaxIoUAssigner with gt_max_assign_all and bbox2delta, DESIGN.md
// section 21; included by monorun_pnp.hip inside its anonymous namespace): two launches for all images of a batch, the maxima and the
// finish.  Contraction is off: every operation is an fp32 one, as include/monorun_assign.h states them.
constexpr int kAssignThreads = 256;     // MR_ASSIGN_THREADS
constexpr int kAssignMaxGt = 256;       // MR_ASSIGN_MAX_GT
constexpr int kAssignMaxIgnore = 256;   // MR_ASSIGN_MAX_IGNORE
constexpr int kAssignMaxImages = 65535; // MR_ASSIGN_MAX_IMAGES

struct AssignArgs {
    const float *boxes; long long image_stride; int box_stride;
    const uint8_t *valid; const int *counts;
    int N, B;
    const float *gt; const int *gt_offsets; const int *gt_labels; int max_gt;
    const float *ign; const int *ign_offsets; int max_ign;
    float pos_thr, neg_thr, min_pos, ign_thr; int low_quality;
    float mean[4], std[4];
    float *max_overlap; int *argmax; uint8_t *ignored; float *gt_max; int *gt_ind; int *label; float *deltas;
    unsigned *keys;                     // (N, max_gt): 0 = none, else the bit pattern of gt_max + 1
};

// torch's max / min: a NaN operand is the result (fmaxf drops it).
__device__ __forceinline__ float assign_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float assign_min(float a, float b) { return (a <= b || a != a) ? a : b; }

// The rule's intersection of boxes a and b: ONE copy, which both overlaps, both kernels and so the `==` of the finish go through.
__device__ __forceinline__ float assign_intersection(const float4 a, const float4 b) {
#pragma clang fp contract(off)
    const float w = assign_max(assign_min(a.z, b.z) - assign_max(a.x, b.x), 0.0f);
    const float h = assign_max(assign_min(a.w, b.w) - assign_max(a.y, b.y), 0.0f);
    return w * h;
}
__device__ __forceinline__ float assign_area(const float4 a) {
#pragma clang fp contract(off)
    return (a.z - a.x) * (a.w - a.y);
}
__device__ __forceinline__ float assign_iou(const float4 a, float area_a, const float4 b) {
#pragma clang fp contract(off)
    const float inter = assign_intersection(a, b);
    return inter / assign_max((area_a + assign_area(b)) - inter, 1e-6f);
}
__device__ __forceinline__ float assign_iof(const float4 a, float area_a, const float4 b) {
#pragma clang fp contract(off)
    return assign_intersection(a, b) / assign_max(area_a, 1e-6f);
}

// The count of image n as both kernels read it: offsets' difference, cut to [0, cap].
__device__ __forceinline__ int assign_count(const int *offsets, int n, int cap) {
    return offsets ? min(max(offsets[n + 1] - offsets[n], 0), cap) : 0;
}

// The first `count` rows of `src` from row `first` on into LDS, by the whole block.
__device__ __forceinline__ void assign_stage(float4 *dst, const float *src, long long first, int count) {
    for (int i = threadIdx.x; i < count; i += kAssignThreads) {
        const float *p = src + (first + i) * 4;
        dst[i] = make_float4(p[0], p[1], p[2], p[3]);
    }
}

__device__ __forceinline__ bool assign_present(const AssignArgs &a, int n, int b) {
    if (b >= a.B) return false;
    if (a.counts && b >= a.counts[n]) return false;
    return !a.valid || a.valid[(long long)n * a.B + b] != 0;
}

__device__ __forceinline__ float4 assign_box(const AssignArgs &a, int n, int b) {
    const float *p = a.boxes + (long long)n * a.image_stride + (long long)b * a.box_stride;
    return make_float4(p[0], p[1], p[2], p[3]);
}

// gt_max's key: 0 for an overlap that raises nothing (negative: an ignored box; NaN), else its bit pattern + 1 (a zero of either sign: 1).
__device__ __forceinline__ unsigned assign_key(float ov) {
    return ov > 0.0f ? __float_as_uint(ov) + 1u : (ov == 0.0f ? 1u : 0u);
}
__device__ __forceinline__ float assign_unkey(unsigned k) { return k ? __uint_as_float(k - 1u) : -1.0f; }

// grid (blocks of 256 boxes, image).  One thread per box: the ignore test, then the row of overlaps with the running maximum; per ground
// truth the overlaps' keys are reduced over the wave, over the block's waves in LDS and over the blocks by one atomicMax per block.
__global__ void __launch_bounds__(kAssignThreads) assign_max_kernel(const AssignArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 gt[kAssignMaxGt];
    __shared__ float4 ign[kAssignMaxIgnore];
    __shared__ unsigned key[kAssignMaxGt];
    const int n = blockIdx.y, b = blockIdx.x * kAssignThreads + threadIdx.x;
    const int G = assign_count(a.gt_offsets, n, a.max_gt);
    const int I = (a.ign_thr > 0.0f && G > 0) ? assign_count(a.ign_offsets, n, a.max_ign) : 0;
    if (G > 0) assign_stage(gt, a.gt, a.gt_offsets[n], G);
    if (I > 0) assign_stage(ign, a.ign, a.ign_offsets[n], I);
    for (int i = threadIdx.x; i < G; i += kAssignThreads) key[i] = 0u;
    __syncthreads();
    const bool present = assign_present(a, n, b);
    float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (present) box = assign_box(a, n, b);
    const float area = assign_area(box);
    bool ignored = false;
    if (present && I > 0) {
        float worst = -1.0f;
        for (int i = 0; i < I; ++i) {
            const float f = assign_iof(box, area, ign[i]);
            if (f > worst) worst = f;
        }
        ignored = worst > a.ign_thr;
    }
    float best = G > 0 ? -1.0f : 0.0f;
    int arg = 0;
    const bool live = present && !ignored;
    for (int i = 0; i < G; ++i) {               // G is uniform over the block: every lane takes part in the shuffles
        const float ov = live ? assign_iou(box, area, gt[i]) : -1.0f;
        if (ov > best) { best = ov; arg = i; }
        unsigned k = live ? assign_key(ov) : 0u;
        for (int d = 32; d; d >>= 1) k = max(k, (unsigned)__shfl_xor((int)k, d));
        if ((threadIdx.x & 63) == 0 && k) atomicMax(&key[i], k);
    }
    if (b < a.B) {
        const long long o = (long long)n * a.B + b;
        a.max_overlap[o] = present ? best : 0.0f;
        a.argmax[o] = arg;
        a.ignored[o] = ignored ? 1 : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < G; i += kAssignThreads)
        if (key[i]) atomicMax(&a.keys[(long long)n * a.max_gt + i], key[i]);
}

// The same grid.  Steps 4 to 6 and the regression target; block 0 of an image also writes its gt_max.
__global__ void __launch_bounds__(kAssignThreads) assign_finish_kernel(const AssignArgs a) {
#pragma clang fp contract(off)
    __shared__ float4 gt[kAssignMaxGt];
    __shared__ float gmax[kAssignMaxGt];
    const int n = blockIdx.y, b = blockIdx.x * kAssignThreads + threadIdx.x;
    const int G = assign_count(a.gt_offsets, n, a.max_gt);
    const long long first = G > 0 ? a.gt_offsets[n] : 0;
    if (G > 0) assign_stage(gt, a.gt, first, G);
    for (int i = threadIdx.x; i < G; i += kAssignThreads) {
        const float m = assign_unkey(a.keys[(long long)n * a.max_gt + i]);
        gmax[i] = m;
        if (blockIdx.x == 0 && a.gt_max) a.gt_max[first + i] = m;
    }
    __syncthreads();
    if (b >= a.B) return;
    const long long o = (long long)n * a.B + b;
    const bool present = assign_present(a, n, b);
    int ind = -1;
    float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (present && G == 0) ind = 0;
    if (present && G > 0) {
        box = assign_box(a, n, b);
        const float mo = a.max_overlap[o];
        if (mo >= 0.0f && mo < a.neg_thr) ind = 0;
        if (mo >= a.pos_thr) ind = a.argmax[o] + 1;
        if (a.low_quality) {
            const bool ignored = a.ignored[o] != 0;
            const float area = assign_area(box);
            for (int i = 0; i < G; ++i) {
                const float ov = ignored ? -1.0f : assign_iou(box, area, gt[i]);
                if (ov == gmax[i] && gmax[i] >= a.min_pos) ind = i + 1;
            }
        }
    }
    a.gt_ind[o] = ind;
    if (a.label) a.label[o] = ind > 0 ? (a.gt_labels ? a.gt_labels[first + ind - 1] : 0) : -1;
    if (a.deltas) {
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ind > 0) {
            const float4 g = gt[ind - 1];
            const float px = (box.x + box.z) * 0.5f, py = (box.y + box.w) * 0.5f, pw = box.z - box.x, ph = box.w - box.y;
            const float gx = (g.x + g.z) * 0.5f, gy = (g.y + g.w) * 0.5f, gw = g.z - g.x, gh = g.w - g.y;
            d[0] = (gx - px) / pw; d[1] = (gy - py) / ph; d[2] = logf(gw / pw); d[3] = logf(gh / ph);
            for (int k = 0; k < 4; ++k) d[k] = (d[k] - a.mean[k]) / a.std[k];
        }
        for (int k = 0; k < 4; ++k) a.deltas[o * 4 + k] = d[k];     // no alignment is asked of the caller's array
    }
}
