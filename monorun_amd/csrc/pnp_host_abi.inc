// include/monorun_pnp.h, the reference's host-buffer C entry points (ext.h:1-43, pnp_uncert_cpu.cpp:245-377) and the batched form of the
// two 7-parameter ones.
// ---- host-buffer entry points of the reference's C ABI (ext.h).  Per device: one private non-blocking stream, one pinned
// host staging buffer and one device buffer, grown on demand and kept; a call is one async H2D copy, the kernel and one async
// D2H copy on that stream followed by a single hipStreamSynchronize (no default-stream launch, no pageable copies, no
// allocation in the steady state).  Calls on the same device serialise on the stage's mutex (the reference invokes these
// serially, pnp_uncert_cpu.py:180-191); calls on different devices run concurrently.
struct HostStage {
    std::mutex mu;
    hipStream_t st = nullptr;
    void *dbuf = nullptr, *hbuf = nullptr;
    size_t cap = 0;
};
static HostStage g_stage[kMaxDevices];

// returns the locked stage of the current device with room for `bytes` in both buffers, or nullptr (lock not held)
static HostStage *stage_acquire(size_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { g_last_hip_error = (int)hipGetLastError(); return nullptr; }
    HostStage *s = &g_stage[dev];
    s->mu.lock();
    bool ok = true;
    if (!s->st) ok = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) == hipSuccess;
    if (ok && bytes > s->cap) {
        const size_t want = bytes < 4096 ? 4096 : bytes + bytes / 2;
        if (s->dbuf) (void)hipFree(s->dbuf);
        if (s->hbuf) (void)hipHostFree(s->hbuf);
        s->dbuf = s->hbuf = nullptr; s->cap = 0;
        ok = hipMalloc(&s->dbuf, want) == hipSuccess && hipHostMalloc(&s->hbuf, want, hipHostMallocDefault) == hipSuccess;
        if (ok) s->cap = want;
    }
    if (!ok) { g_last_hip_error = (int)hipGetLastError(); s->mu.unlock(); return nullptr; }
    return s;
}

// The reference's per-object entry point (ext.h:1-13).  Host fp64 buffers; one object; blocking.
void pnp_uncert(double *pts2d, double *pts3d, double *wgt2d, double *K, double *init_pose,
                int *result_val, double *result_pose, double *result_cov, double *result_tr,
                int pn, double *clips) {
    *result_val = 0;
    memcpy(result_pose, init_pose, 4 * sizeof(double));                  // pnp_uncert_cpu.cpp:259
    *result_tr = 0.0;
    if (pn < 1 || pn > 65535) return;
    const int P = pn < 4 ? 4 : pn;
    // staging, in doubles: [pts2d 2P | pts3d 3P | wgt 2P | K 9 | ur 2 | vr 2 | init 4 || pose64 4 | cov64 16 | tr64 1 | valid (u8, 8 bytes)]
    //                      + [pose 4 | cov 16 | tr 1] floats (written by the kernel, not read back)
    const size_t nin = (size_t)7 * P + 9 + 2 + 2 + 4, nout = 4 + 16 + 1 + 1;
    const size_t bytes = (nin + nout) * sizeof(double) + 24 * sizeof(float);
    HostStage *sg = stage_acquire(bytes);
    if (!sg) return;
    std::lock_guard<std::mutex> lk(sg->mu, std::adopt_lock);
    double *h = (double *)sg->hbuf, *d = (double *)sg->dbuf;
    double *h2 = h, *h3 = h2 + 2 * P, *hw = h3 + 3 * P, *hK = hw + 2 * P, *hur = hK + 9, *hvr = hur + 2, *hin = hvr + 2;
    memcpy(h2, pts2d, sizeof(double) * 2 * pn); memcpy(h3, pts3d, sizeof(double) * 3 * pn); memcpy(hw, wgt2d, sizeof(double) * 2 * pn);
    for (int p = pn; p < P; ++p) { h2[2 * p] = h2[2 * p + 1] = 0.0; h3[3 * p] = h3[3 * p + 1] = 0.0; h3[3 * p + 2] = 1.0; hw[2 * p] = hw[2 * p + 1] = 0.0; }   // padded points carry zero weight
    memcpy(hK, K, sizeof(double) * 9);
    hur[0] = clips[1]; hur[1] = clips[2]; hvr[0] = clips[3]; hvr[1] = clips[4];
    memcpy(hin, init_pose, sizeof(double) * 4);
    if (hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    PnpArgs a;
    memset(&a, 0, sizeof a);
    a.x2d = d; a.x3d = d + 2 * P; a.istd = d + 5 * P;
    a.s2[0] = 0; a.s2[1] = 2; a.s2[2] = 1; a.sw[0] = 0; a.sw[1] = 2; a.sw[2] = 1; a.s3[0] = 0; a.s3[1] = 3; a.s3[2] = 1;
    a.K = d + 7 * P; a.K_stride = 0; a.K_f64 = 1;
    a.ur = d + 7 * P + 9; a.vr = d + 7 * P + 11; a.r_stride = 0; a.r_f64 = 1;
    a.init_pose = d + 7 * P + 13;
    double *dout = d + nin;
    a.pose64 = dout; a.cov64 = dout + 4; a.tr64 = dout + 20; a.valid = (uint8_t *)(dout + 21);
    float *df = (float *)(dout + nout);
    a.pose = df; a.cov = df + 4; a.tr = df + 20;
    a.B = 1; a.P = P; a.z_min = clips[0]; a.istd_thres = 0.f; a.inlier_opt_only = 0;
    a.flags = MR_NO_ISTD_MASK | (result_cov ? MR_COV_CERES : MR_COV_NONE);
    a.mean_mode = MR_MEAN_SEQUENTIAL;
    int wpo = 1; while (wpo < 8 && P >= 64 * wpo * 2) wpo *= 2;
    if (launch_wpo<double>(a, wpo, sg->st) != MR_OK) return;
    double *ho = h + nin;
    if (hipMemcpyAsync(ho, dout, nout * sizeof(double), hipMemcpyDeviceToHost, sg->st) != hipSuccess ||
        hipStreamSynchronize(sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    const uint8_t ok = *(const uint8_t *)(ho + 21);
    memcpy(result_pose, ho, 4 * sizeof(double));
    *result_tr = ho[20];
    *result_val = ok ? 1 : 0;
    if (ok && result_cov) memcpy(result_cov, ho + 4, 16 * sizeof(double));
}

// The 7-parameter entry points of the reference's C ABI (ext.h:15-43).  Host fp64 buffers; one object; blocking.
static void noc_host(int full_cov, double *pts2d, double *pts3d, double *wgt2d, double *logdim, double *logdim_wgt, double *K,
                     double *init_dimpose, int *result_val, double *result_dimpose, int pn, double *clips, double delta) {
    *result_val = 0;
    memcpy(result_dimpose, init_dimpose, 7 * sizeof(double));            // pnp_uncert_cpu.cpp:309,351
    if (pn < 0) return;
    const int ws = full_cov ? 3 : 2;
    // staging, in doubles: [pts2d 2n | pts3d 3n | wgt ws*n | logdim 3 | logdim_wgt 3 | K 9 | init 7 | clips 5 || out 7 | val (int, 8 bytes)]
    const size_t n = (size_t)pn;
    const size_t nin = (2 + 3 + ws) * n + 3 + 3 + 9 + 7 + 5, nout = 7 + 1;
    HostStage *sg = stage_acquire((nin + nout) * sizeof(double));
    if (!sg) return;
    std::lock_guard<std::mutex> lk(sg->mu, std::adopt_lock);
    double *h = (double *)sg->hbuf, *d = (double *)sg->dbuf;
    double *q = h;
    memcpy(q, pts2d, sizeof(double) * 2 * n); q += 2 * n;
    memcpy(q, pts3d, sizeof(double) * 3 * n); q += 3 * n;
    memcpy(q, wgt2d, sizeof(double) * ws * n); q += ws * n;
    memcpy(q, logdim, sizeof(double) * 3); q += 3;
    memcpy(q, logdim_wgt, sizeof(double) * 3); q += 3;
    memcpy(q, K, sizeof(double) * 9); q += 9;
    memcpy(q, init_dimpose, sizeof(double) * 7); q += 7;
    memcpy(q, clips, sizeof(double) * 5);
    if (hipMemcpyAsync(d, h, nin * sizeof(double), hipMemcpyHostToDevice, sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    NocArgs a;
    memset(&a, 0, sizeof a);
    a.pts2d = d; a.pts3d = d + 2 * n; a.wgt2d = d + 5 * n; a.logdim = d + (5 + ws) * n; a.logdim_wgt = a.logdim + 3; a.K = a.logdim + 6;
    a.init = a.logdim + 15; a.clips = a.logdim + 22; a.out_dimpose = d + nin; a.out_val = (int *)(d + nin + 7); a.out_diag = nullptr;
    a.K_batch = 1; a.clips_batch = 1; a.B = 1;
    a.delta = delta; a.pn = pn; a.full_cov = full_cov;
    hipLaunchKernelGGL(pnp_noc_kernel, dim3(1), dim3(256), kNocLds, sg->st, a);
    if (hipGetLastError() != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    double *ho = h + nin;
    if (hipMemcpyAsync(ho, d + nin, nout * sizeof(double), hipMemcpyDeviceToHost, sg->st) != hipSuccess ||
        hipStreamSynchronize(sg->st) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); return; }
    memcpy(result_dimpose, ho, 7 * sizeof(double));
    *result_val = *(const int *)(ho + 7);
}

void pnp_noc_uncert(double *pts2d, double *pts3d, double *wgt2d, double *logdim, double *logdim_wgt, double *K,
                    double *init_dimpose, int *result_val, double *result_dimpose, int pn, double *clips, double delta) {
    noc_host(0, pts2d, pts3d, wgt2d, logdim, logdim_wgt, K, init_dimpose, result_val, result_dimpose, pn, clips, delta);
}

void pnp_noc_cov_uncert(double *pts2d, double *pts3d, double *wgt2d, double *logdim, double *logdim_wgt, double *K,
                        double *init_dimpose, int *result_val, double *result_dimpose, int pn, double *clips, double delta) {
    noc_host(1, pts2d, pts3d, wgt2d, logdim, logdim_wgt, K, init_dimpose, result_val, result_dimpose, pn, clips, delta);
}

// Batched form of the two 7-parameter solvers (device fp64 buffers, one workgroup per object; pnp_noc_kernel.inc)
int mr_pnp_noc_batched(int full_cov, const double *pts2d, const double *pts3d, const double *wgt2d, const double *logdim, const double *logdim_wgt,
                       const double *K, int K_batch, const double *init_dimpose, const double *clips, int clips_batch, double delta, int B, int pn,
                       double *result_dimpose, int32_t *result_val, double *diag, void *stream) {
    if (B < 0 || pn < 0 || (K_batch != 1 && K_batch != B) || (clips_batch != 1 && clips_batch != B)) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if ((pn > 0 && (!pts2d || !pts3d || !wgt2d)) || !logdim || !logdim_wgt || !K || !init_dimpose || !clips || !result_dimpose || !result_val) return MR_ERR_BAD_ARGUMENT;
    NocArgs a;
    memset(&a, 0, sizeof a);
    a.pts2d = pts2d; a.pts3d = pts3d; a.wgt2d = wgt2d; a.logdim = logdim; a.logdim_wgt = logdim_wgt; a.K = K; a.init = init_dimpose; a.clips = clips;
    a.K_batch = K_batch; a.clips_batch = clips_batch; a.delta = delta; a.pn = pn; a.full_cov = full_cov ? 1 : 0; a.B = B;
    a.out_dimpose = result_dimpose; a.out_val = (int *)result_val; a.out_diag = diag;
    hipLaunchKernelGGL(pnp_noc_kernel, dim3(B), dim3(256), kNocLds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
