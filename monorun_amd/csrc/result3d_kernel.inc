// result3d_kernel.inc — the per-image tail after the score head in ONE launch (included by monorun_pnp.hip after consumers_kernel.inc,
// whose NMS routine it calls): the (n, 8) rows of monorun_roi_head.py:606-617, their split by class, xywhr2xyxyr, the rotated-BEV NMS
// per class and the gather of the kept 3-D rows and 2-D boxes (monorun_roi_head.py:552-565), class-grouped and padded.  DESIGN.md §24.
constexpr int kResult3dMaxN = 512;          // MR_RESULT3D_MAX_N: nms_group_lds_scan's group cap (16 mask words, one per lane of a wave)
constexpr int kResult3dMaxClasses = 16;     // MR_RESULT3D_MAX_CLASSES
constexpr int kResult3dThreads = 256;       // MR_RESULT3D_THREADS: nms_group_lds_scan strides by 256

// LDS of a launch over N rows: a class may hold all of them.  The NMS routine's arrays, then the members' rows; the routine's 16 spare
// bytes hold the waves' member counts, then the kept count.
__host__ __device__ constexpr size_t result3d_lds(int n, int np2) { return nms_group_lds(n, np2) + (size_t)n * 4; }

struct Result3dArgs {
    const float *dimensions, *yaw, *t_vec, *scores, *det_bboxes;
    const long long *labels;
    int N, C;
    float thr;
    float *out3d, *out2d;
    long long *keep_local, *keep_row;
    int *num_keep, *num_in_class;
};

__global__ void __launch_bounds__(256) result3d_nms_kernel(Result3dArgs a) {
    const int c = blockIdx.x, tid = threadIdx.x, N = a.N;
    extern __shared__ __align__(16) unsigned char smem[];
    // the carve for N members; the class's n <= N members use the front of each array
    const int np2_max = mr_nms_padded(N);
    int *scount = (int *)(smem + nms_group_lds(N, np2_max) - 16);      // [4]
    int *smember = (int *)(smem + nms_group_lds(N, np2_max));          // [N] row of the member with local index i

    // 1. the members in ascending row order: a member's local index is the number of earlier rows of its class
    int n = 0;
    for (int base = 0; base < N; base += 256) {
        const int r = base + tid;
        const bool mine = r < N && a.labels[r] == (long long)c;
        const unsigned long long vote = __ballot(mine);
        const int lane = tid & 63, wave = tid >> 6;
        if (lane == 0) scount[wave] = __popcll(vote);
        __syncthreads();
        int before = n, total = n;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int cw = scount[w]; total += cw; if (w < wave) before += cw; }
        if (mine) smember[before + __popcll(vote & ((1ull << lane) - 1ull))] = r;
        n = total;
        __syncthreads();
    }

    int kept = 0;
    if (n > 0) {                                             // uniform: every thread has the same n
        const int np2 = mr_nms_padded(n);
        float *skey = (float *)smem;                         // [np2]
        int *sidx = (int *)(skey + np2);                     // [np2]
        NmsBox *sbox = (NmsBox *)(sidx + np2);               // [n] in sorted order
        unsigned *srow = (unsigned *)(sbox + n);             // [n][(n + 31) / 32]
        // the members' scores in local order, staged where the boxes go after the sort
        float *sscore = (float *)sbox;
        for (int i = tid; i < n; i += 256) sscore[i] = a.scores[smember[i]];
        __syncthreads();
        int *skept = (int *)skey;                            // [n] local indices of the kept, in kept order; the keys are dead once the sort is done
        kept = nms_group_lds_scan(
            skey, sidx, sbox, srow, n, np2, sscore, a.thr, tid,
            [&](int j) {
                // 2. xywhr2xyxyr of [x, z, l, w, ry]: half = size / 2, centre -+ half, each rounded to fp32 on its own
                const int r = smember[j];
                const float cx = a.t_vec[r * 3], cy = a.t_vec[r * 3 + 2];
                const float hl = a.dimensions[r * 3] * 0.5f, hw = a.dimensions[r * 3 + 2] * 0.5f;
                return nms_make_box(__fsub_rn(cx, hl), __fsub_rn(cy, hw), __fadd_rn(cx, hl), __fadd_rn(cy, hw), a.yaw[r]);
            },
            [&](int k, int i) { skept[k] = sidx[i]; });
        if (tid == 0) scount[0] = kept;
        __syncthreads();
        kept = scount[0];
        for (int k = tid; k < kept; k += 256) {
            const int local = skept[k], r = smember[local];
            const long long o = (long long)c * N + k;
            const float4 lo = make_float4(a.dimensions[r * 3], a.dimensions[r * 3 + 1], a.dimensions[r * 3 + 2], a.t_vec[r * 3]);
            const float4 hi = make_float4(a.t_vec[r * 3 + 1], a.t_vec[r * 3 + 2], a.yaw[r], a.scores[r]);
            float4 *o3 = (float4 *)(a.out3d + o * 8);
            o3[0] = lo; o3[1] = hi;
#pragma unroll
            for (int q = 0; q < 5; ++q) a.out2d[o * 5 + q] = a.det_bboxes[r * 5 + q];
            a.keep_local[o] = (long long)local;
            a.keep_row[o] = (long long)r;
        }
    }
    // the places past the kept: NaN and -1, so that every element is stored exactly once
    const float nanf_ = __int_as_float(0x7fc00000);
    for (int k = kept + tid; k < N; k += 256) {
        const long long o = (long long)c * N + k;
        float4 *o3 = (float4 *)(a.out3d + o * 8);
        o3[0] = o3[1] = make_float4(nanf_, nanf_, nanf_, nanf_);
#pragma unroll
        for (int q = 0; q < 5; ++q) a.out2d[o * 5 + q] = nanf_;
        a.keep_local[o] = -1;
        a.keep_row[o] = -1;
    }
    if (tid == 0) { a.num_keep[c] = kept; a.num_in_class[c] = n; }
}
