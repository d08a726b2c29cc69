// include/monorun_pnp.h, the library and its diagnostics: version, error strings, device count, the wave rule (pick_wpo, host_launch.inc)
// and the stream-overlap probe.  No counterpart in the reference.  Included inside monorun_pnp.hip's extern "C" block, like every *_abi.inc.
int mr_pnp_version(void) { return MR_PNP_VERSION; }

const char *mr_pnp_error_string(int code) {
    switch (code) {
        case MR_OK: return "ok";
        case MR_ERR_BAD_ARGUMENT: return "bad argument";
        case MR_ERR_UNSUPPORTED: return "unsupported configuration (P too large for LDS, or unknown dtype)";
        case MR_ERR_HIP: return "HIP runtime error (see mr_pnp_last_hip_error)";
        case MR_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown error";
    }
}

int mr_pnp_last_hip_error(void) { return g_last_hip_error; }

int mr_pnp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// waves per object the library would pick for a launch of `objects_in_flight` objects x P points on the current device (pick_wpo): lets
// a caller that keeps several launches in flight apply the library's own rule to ALL the objects on the chip (PnPPipeline.flags_for)
int mr_pick_waves(int objects_in_flight, int P) {
    if (objects_in_flight < 1 || P < 4) return MR_ERR_BAD_ARGUMENT;
    return pick_wpo(objects_in_flight, P, 0);
}

// Occupies one wavefront of the device for `microseconds` (100 MHz constant clock).  PnPPipeline uses it to find out which of
// its streams the runtime really runs side by side: HIP maps streams onto a small number of hardware queues (4 per priority level
// by default) and two streams that share a queue serialise.
int mr_spin(int microseconds, void *stream) {
    if (microseconds < 0 || microseconds > 1000000) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long)microseconds * 100);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
