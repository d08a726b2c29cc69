// Development aids of the tests and the profiling tools: exported, in no public header.
// development aid (not in the public header): device buffer of (B,10) u64 cycle stamps, or NULL to disable
void mr_pnp_debug_set_stamps(unsigned long long *dev_ptr) { g_stamps = dev_ptr; }
#ifdef MR_DEBUG_STAMPS
// -DMR_DEBUG_STAMPS builds only: device buffer of (B,24) u64 stamps of the consensus launches (EPC_STAMP, tools/gpu_consensus_stamps.py), or NULL
void mr_pnp_debug_set_consensus_stamps(unsigned long long *dev_ptr) { g_cons_stamps = dev_ptr; }
#endif

// development aids for the tests (not in the public header):
// waves per object of the LM / covariance launch over `objects` objects x P points of `in_dtype` with `flags` (MR_WAVES bits honoured),
// after the default flow's initialiser when `after_init` is set (mr_pnp_uncert_from_init_* / _from_epnp_grouped), else the fast mode's
int mr_debug_launch_waves(int objects, int P, int in_dtype, int flags, int after_init) {
    if (objects < 1 || P < 4 || P > 64 * kMaxChunks || (in_dtype != MR_F32 && in_dtype != MR_F16 && in_dtype != MR_F64)) return MR_ERR_BAD_ARGUMENT;
    static const uint8_t any_mask = 0;
    PnpArgs a;
    memset(&a, 0, sizeof a);
    a.B = objects; a.P = P; a.flags = flags;
    a.init_mask = after_init ? &any_mask : nullptr;
    return lm_launch_waves(a, flags, in_dtype);
}

// block_sum_packed<wpo, 10> on `partials` (device, 64 wpo x 10 doubles, lane-major) -> `out` (device, wpo x 10: every wave's totals)
int mr_debug_block_sum(int wpo, const double *partials, double *out, void *stream) {
    if (!partials || !out) return MR_ERR_BAD_ARGUMENT;
    hipStream_t st = (hipStream_t)stream;
    switch (wpo) {
        case 1: hipLaunchKernelGGL(block_sum_probe_kernel<1>, dim3(1), dim3(64), 0, st, partials, out); break;
        case 2: hipLaunchKernelGGL(block_sum_probe_kernel<2>, dim3(1), dim3(128), 0, st, partials, out); break;
        case 3: hipLaunchKernelGGL(block_sum_probe_kernel<3>, dim3(1), dim3(192), 0, st, partials, out); break;
        case 4: hipLaunchKernelGGL(block_sum_probe_kernel<4>, dim3(1), dim3(256), 0, st, partials, out); break;
        case 8: hipLaunchKernelGGL(block_sum_probe_kernel<8>, dim3(1), dim3(512), 0, st, partials, out); break;
        default: return MR_ERR_BAD_ARGUMENT;
    }
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
