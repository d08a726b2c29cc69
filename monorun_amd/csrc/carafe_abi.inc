// include/monorun_carafe.h: the NOC head trunk's upsampler, CARAFEPack's normaliser + reassembly fused (mmcv.ops.carafe)
static int carafe_fill(CarafeArgs &a, int n, int C, int h, int w, int k, int G, int s) {
    static_assert(kCarafeTile == MR_CARAFE_TILE && kCarafeChunk == MR_CARAFE_CHUNK, "the header states the tiling");
    if (n < 0 || C < 1 || h < 1 || w < 1 || G < 1 || C % G != 0) return MR_ERR_BAD_ARGUMENT;
    if (!(k == 1 || k == 3 || k == 5 || k == 7) || !(s == 1 || s == 2 || s == 4)) return MR_ERR_UNSUPPORTED;
    // offsets inside one RoI are 32-bit in the kernels: its channels x output pixels and its logits must fit
    if ((long long)C * h * s * w * s > 0x7fffffffLL || (long long)G * k * k * s * s * h * w > 0x7fffffffLL) return MR_ERR_UNSUPPORTED;
    memset(&a, 0, sizeof a);
    a.N = n; a.C = C; a.H = h; a.W = w; a.G = G; a.s = s; a.ls = s == 4 ? 2 : s == 2 ? 1 : 0;
    a.Cg = C / G; a.cpg = (a.Cg + kCarafeChunk - 1) / kCarafeChunk;
    a.tiles_x = (w + kCarafeTile - 1) / kCarafeTile; a.tiles_y = (h + kCarafeTile - 1) / kCarafeTile;
    return MR_OK;
}

// one of the three kernels at the up_kernel the arguments name: `which` 0 forward, 1 backward masks / grad_m, 2 backward grad_x
#define MR_CARAFE_LAUNCH(K) do { \
        if (which == 0) hipLaunchKernelGGL(carafe_pack_forward_kernel<K>, dim3(nb), dim3(kCarafeThreads), 0, st, a); \
        else if (which == 1) hipLaunchKernelGGL(carafe_pack_backward_mask_kernel<K>, dim3(nb), dim3(kCarafeThreads), 0, st, a); \
        else hipLaunchKernelGGL(carafe_pack_backward_input_kernel<K>, dim3(nb), dim3(kCarafeThreads), 0, st, a); \
    } while (0)
static int carafe_launch(int which, int k, long long blocks, hipStream_t st, const CarafeArgs &a) {
    unsigned nb;
    if (grid_1d(blocks, 1, nb) != MR_OK) return MR_ERR_UNSUPPORTED;
    switch (k) {
        case 1: MR_CARAFE_LAUNCH(1); break;
        case 3: MR_CARAFE_LAUNCH(3); break;
        case 5: MR_CARAFE_LAUNCH(5); break;
        default: MR_CARAFE_LAUNCH(7); break;
    }
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
#undef MR_CARAFE_LAUNCH

int mr_carafe_pack_forward(const float *x, const float *m, int n, int channels, int h, int w, int up_kernel, int up_group, int scale_factor,
                           float *out, void *stream) {
    CarafeArgs a;
    const int rc = carafe_fill(a, n, channels, h, w, up_kernel, up_group, scale_factor);
    if (rc != MR_OK) return rc;
    if (n == 0) return MR_OK;
    if (!x || !m || !out) return MR_ERR_BAD_ARGUMENT;
    a.x = x; a.m = m; a.out = out;
    return carafe_launch(0, up_kernel, (long long)n * a.G * a.cpg * a.tiles_x * a.tiles_y, (hipStream_t)stream, a);
}

size_t mr_carafe_backward_workspace_bytes(int n, int channels, int h, int w, int up_kernel, int up_group, int scale_factor) {
    CarafeArgs a;
    if (carafe_fill(a, n, channels, h, w, up_kernel, up_group, scale_factor) != MR_OK) return 0;
    return sizeof(float) * (size_t)n * up_group * up_kernel * up_kernel * ((size_t)h * scale_factor) * ((size_t)w * scale_factor);
}

int mr_carafe_pack_backward(const float *x, const float *m, const float *grad_out, int n, int channels, int h, int w, int up_kernel,
                            int up_group, int scale_factor, void *workspace, size_t workspace_bytes, float *grad_x, float *grad_m,
                            void *stream) {
    CarafeArgs a;
    const int rc = carafe_fill(a, n, channels, h, w, up_kernel, up_group, scale_factor);
    if (rc != MR_OK) return rc;
    if (n == 0 || (!grad_x && !grad_m)) return MR_OK;
    if (!x || !m || !grad_out) return MR_ERR_BAD_ARGUMENT;
    if (grad_x && (!workspace || ((uintptr_t)workspace & 3) ||
                   workspace_bytes < mr_carafe_backward_workspace_bytes(n, channels, h, w, up_kernel, up_group, scale_factor)))
        return MR_ERR_BAD_ARGUMENT;
    a.x = x; a.m = m; a.go = grad_out; a.gx = grad_x; a.gm = grad_m; a.wn = grad_x ? (float *)workspace : nullptr;
    const long long tiles = (long long)a.tiles_x * a.tiles_y;
    const int r1 = carafe_launch(1, up_kernel, (long long)n * a.G * tiles * scale_factor * scale_factor, (hipStream_t)stream, a);
    if (r1 != MR_OK || !grad_x) return r1;
    return carafe_launch(2, up_kernel, (long long)n * a.G * a.cpg * tiles, (hipStream_t)stream, a);
}
