// include/monorun_global.h: the global head's Monte-Carlo eval forward, factored over the channel mask (fc_extractor_monte_carlo.py:41-63)
static int global_head_check(int n, int C, int A, int F, int J, int S) {
    if (n < 0 || C < 1 || A < 1 || F < 1 || J < 1 || S < 2) return MR_ERR_BAD_ARGUMENT;
    if (C > MR_GLOBAL_MAX_CHANNELS || A > MR_GLOBAL_MAX_CHANNELS || F > MR_GLOBAL_MAX_CHANNELS || J > MR_GLOBAL_MAX_OUT || S > MR_GLOBAL_MAX_SAMPLES)
        return MR_ERR_UNSUPPORTED;
    const long long lim = 0x7fffffffLL, sn = (long long)S * n, ca = (long long)C * A;
    if (n * ca > lim || F * ca > lim || sn * F > lim || sn * C > lim || sn * J > lim) return MR_ERR_UNSUPPORTED;
    return MR_OK;
}

static size_t global_head_pass_floats(int nc, int C, int F, int J, int S) {
    return (size_t)nc * ((size_t)C * F + 2 * (size_t)S * F + (size_t)S * J);
}

size_t mr_global_head_mc_workspace_bytes(int n, int in_channels, int area, int fc_channels, int out_channels, int num_samples) {
    if (global_head_check(n, in_channels, area, fc_channels, out_channels, num_samples) != MR_OK) return 0;
    return sizeof(float) * global_head_pass_floats(n < kGhChunk ? n : kGhChunk, in_channels, fc_channels, out_channels, num_samples);
}

int mr_global_head_mc_forward(const float *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *w_reg,
                              const float *b_reg, const uint8_t *keep0, const uint8_t *keep1, const uint8_t *keep2, float q0, float q1,
                              int n, int in_channels, int area, int fc_channels, int out_channels, int num_samples, void *workspace,
                              size_t workspace_bytes, float *mean, float *var, float *reg_fc_out, float *samples, void *stream) {
    static_assert(kGhChunk == MR_GLOBAL_CHUNK, "the header states the pass size");
    const int C = in_channels, A = area, F = fc_channels, J = out_channels, S = num_samples;
    const int rc = global_head_check(n, C, A, F, J, S);
    if (rc != MR_OK) return rc;
    if (n == 0) return MR_OK;
    if (!x || !w1 || !b1 || !w2 || !b2 || !w_reg || !b_reg || !keep0 || !keep1 || !keep2 || !workspace || !mean || !var || !reg_fc_out)
        return MR_ERR_BAD_ARGUMENT;
    const int chunk = n < kGhChunk ? n : kGhChunk;
    if (((uintptr_t)workspace & 3) || workspace_bytes < sizeof(float) * global_head_pass_floats(chunk, C, F, J, S)) return MR_ERR_BAD_ARGUMENT;
    GhArgs a;
    a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.wr = w_reg; a.br = b_reg;
    a.keep0 = keep0; a.keep1 = keep1; a.keep2 = keep2; a.q0 = q0; a.q1 = q1;
    a.n = n; a.C = C; a.A = A; a.F = F; a.J = J; a.S = S;
    a.P = (float *)workspace;
    a.h1 = a.P + (size_t)chunk * C * F;
    a.h2 = a.h1 + (size_t)chunk * S * F;
    a.ys = a.h2 + (size_t)chunk * S * F;
    a.mean = mean; a.var = var; a.reg = reg_fc_out; a.samples = samples;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nt = (unsigned)((F + kGhBN - 1) / kGhBN);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        a.i0 = i0; a.nc = n - i0 < chunk ? n - i0 : chunk;
        const unsigned rows = (unsigned)(S * a.nc);
        hipLaunchKernelGGL(gh_p_kernel, dim3(nt, (unsigned)((a.nc + kGhBM - 1) / kGhBM), (unsigned)C), dim3(kGhThreads), 0, st, a);
        hipLaunchKernelGGL(gh_h1_kernel, dim3(nt, (unsigned)((S + kGhBM - 1) / kGhBM), (unsigned)a.nc), dim3(kGhThreads), 0, st, a);
        hipLaunchKernelGGL(gh_h2_kernel, dim3(nt, (rows + kGhBM - 1) / kGhBM, 1), dim3(kGhThreads), 0, st, a);
        hipLaunchKernelGGL(gh_out_kernel, dim3((rows + kGhOutRows - 1) / kGhOutRows), dim3(64 * kGhOutRows), 0, st, a);
        hipLaunchKernelGGL(gh_stats_kernel, dim3((unsigned)a.nc), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return MR_OK;
}
