// include/monorun_pnp.h, the solver launches: the fused 4-DoF PnP (pnp_uncert_cpu.cpp:245-292 batched), the EPnP + RANSAC initialiser
// (pnp_uncert_cpu.py:33-68), the LM launches behind an initialiser, the eigenvalue rule (pnp_uncert.py:77-85), the 6-DoF refinement,
// the exact Hessian (hessian.py:5-64) and the backward.
static int pnp_uncert_launch(
    const CorrIn &in, int in_dtype,
    const float *ransac_thr, const double *init_pose, const uint8_t *init_mask, const uint8_t *init_valid, int B, int P,
    float z_min, float istd_thres, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag, void *stream,
    int ncalls = 1, const PnpCallTable::CallPtrs *calls = nullptr, const EpnpRefitIn *rf = nullptr, const float *calib_logscale = nullptr, float corr_sd = 0.0f) {
    if (B < 0 || P < 4 || P > 64 * kMaxChunks) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !valid || !pose || !tr_radius || (!cov && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    PnpArgs a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.ransac_thr = ransac_thr; a.init_pose = init_pose; a.init_mask = init_mask; a.init_valid = init_valid;
    a.B = B; a.P = P; a.z_min = (double)z_min; a.istd_thres = istd_thres; a.inlier_opt_only = inlier_opt_only; a.flags = flags;
    a.valid = valid; a.pose = pose; a.cov = cov; a.tr = tr_radius; a.mask = inlier_mask; a.diag = diag;
    a.stamps = g_stamps;
    if (calib_logscale && calls && calls[0].cov_calib) { a.calib_logscale = calib_logscale; a.corr_sd = corr_sd; a.cov_calib = calls[0].cov_calib; }      // per call: the table's
    int rc;
    if ((rc = choose_mean_order(a)) != MR_OK) return rc;
    PnpCallTable tbl;
    memset(&tbl, 0, sizeof tbl);
    tbl.ncalls = 1; tbl.group_B = B;
    if (ncalls > 1 || rf) {                             // a launch over the objects of several calls (EXT only): mr_pnp_uncert_from_init_grouped / _from_epnp_grouped
        tbl.ncalls = ncalls; a.B = B * ncalls;
        for (int c = 0; c < ncalls; ++c) tbl.call[c] = calls[c];
    }
    const int wpo = lm_launch_waves(a, flags, in_dtype);
    hipStream_t st = (hipStream_t)stream;
    const PnpCallTable *tp = (ncalls > 1 || rf) ? &tbl : nullptr;
    return with_storage_type(in_dtype, [&](auto t) { return launch_wpo<typename decltype(t)::type>(a, wpo, st, tp, rf); });
}

int mr_pnp_uncert_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const float *ransac_thr, const double *init_pose, int B, int P,
    float z_min, float istd_thres, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag, void *stream) {
    return pnp_uncert_launch({ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch }, in_dtype,
                             ransac_thr, init_pose, nullptr, nullptr, B, P, z_min, istd_thres, inlier_opt_only, flags,
                             valid, pose, cov, tr_radius, inlier_mask, diag, stream);
}

static int epnp_ransac_launch(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *ransac_thr, int B, int P,
    float istd_thres, int flags, int max_iters,
    double *const *init_pose, uint8_t *const *init_mask, uint8_t *const *init_valid, float *const *diag, double *debug_hypotheses,
    void *workspace, size_t workspace_bytes, void *stream) {
    if (ncalls < 1 || ncalls > kEpMaxGroup || B < 0 || P < 4 || P > 64 * kMaxChunks || max_iters < 1 || max_iters > kEpMaxIters) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if ((long long)B * ncalls > 0x7fffffffll / kEpMaxIters) return MR_ERR_UNSUPPORTED;
    if (!x2d || !istd || !x3d || !x2d_strides || !istd_strides || !x3d_strides || !cam_mats || !init_pose || !init_mask || !init_valid) return MR_ERR_BAD_ARGUMENT;
    const CorrIn in{ x2d[0], x2d_strides, istd[0], istd_strides, x3d[0], x3d_strides, cam_mats[0], cam_batch, nullptr, nullptr, 1 };
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    EpnpStageArgs sa;
    memset(&sa, 0, sizeof sa);
    for (int c = 0; c < ncalls; ++c) {
        if (!x2d[c] || !istd[c] || !x3d[c] || !cam_mats[c] || !init_pose[c] || !init_mask[c] || !init_valid[c]) return MR_ERR_BAD_ARGUMENT;
        const CallBias at(c, B, in_dtype);
        if (at.mixed(ransac_thr) || at.mixed(diag)) return MR_ERR_BAD_ARGUMENT;     // all or none
        EpnpCallPtrs &q = sa.call[c];
        q.x2d = at(x2d, x2d_strides); q.istd = at(istd, istd_strides); q.x3d = at(x3d, x3d_strides); q.K = at(cam_mats, cam_batch == 1 ? 0 : 9);
        q.ransac_thr = at(ransac_thr, 1);
        q.init_pose = at(init_pose, 4); q.init_mask = at(init_mask, P); q.init_ok = at(init_valid, 1); q.diag = at(diag, 4);
    }
    if (debug_hypotheses && ncalls != 1) return MR_ERR_BAD_ARGUMENT;
    if ((flags & MR_EPNP_DEFER_REFIT) && !workspace) return MR_ERR_BAD_ARGUMENT;       // the LM launch that finishes the job needs the workspace
    PnpArgs &a = sa.p;
    set_inputs(a, in);
    a.ransac_thr = ransac_thr ? ransac_thr[0] : nullptr;
    a.B = B * ncalls; a.P = P; a.istd_thres = istd_thres; a.flags = flags;
    int rc;
    if ((rc = choose_mean_order(a)) != MR_OK) return rc;
    a.stamps = g_stamps;
#ifdef MR_DEBUG_STAMPS
    sa.cstamps = g_cons_stamps;
#endif
    sa.init_pose = init_pose[0]; sa.init_mask = init_mask[0]; sa.init_ok = init_valid[0]; sa.diag = diag ? diag[0] : nullptr; sa.dbg_hyp = debug_hypotheses; sa.max_iters = max_iters;
    sa.ncalls = ncalls; sa.group_B = B;
    hipStream_t st = (hipStream_t)stream;
    // hypotheses solved for every object before the replayed loop is consulted: MR_EPNP_FIRST_ROUND bits of `flags` (1..30), else the
    // environment variable MR_EPNP_FIRST_ROUND, else by the size of the launch set: 10 up to 2047 objects (one call at a time: the
    // second round is a full latency chain; 8 hypotheses make it idle in 85 % of config-2 batches, 10 in 97 %: 278.6 -> 264.1 us per
    // 1024-object call, 228.9 -> 221.8 at 256, within noise at 100 — profiles/r06_first_round.txt), 3 beyond (several calls grouped
    // or a large batch: the chip is busy, the hypotheses nobody needs are the cost — sets of three calls: 9.6 / 9.9 / 10.3 / 10.3 M solves/s
    // with 6 / 4 / 3 / 2, profiles/r05_epnp_grouped_first_round.txt).  Changes the work, never a result.
    static const int first_env = [] { const char *e = getenv("MR_EPNP_FIRST_ROUND"); const int v = e ? atoi(e) : 0; return v < 1 ? 0 : (v > 30 ? 30 : v); }();
    const int first_bits = (flags & MR_EPNP_FIRST_ROUND_MASK) >> MR_EPNP_FIRST_ROUND_SHIFT;
    const int first_round = first_bits ? (first_bits > 30 ? 30 : first_bits) : (first_env ? first_env : ((long long)B * ncalls >= 2048 ? 3 : 10));
    return with_storage_type(in_dtype, [&](auto t) { return launch_epnp_stages<typename decltype(t)::type>(sa, workspace, workspace_bytes, first_round, st); });
}

int mr_epnp_ransac_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *ransac_thr, int B, int P,
    float istd_thres, int flags, int max_iters,
    double *init_pose, uint8_t *init_mask, uint8_t *init_valid, float *diag, double *debug_hypotheses,
    void *workspace, size_t workspace_bytes, void *stream) {
    return epnp_ransac_launch(1, &x2d, x2d_strides, &istd, istd_strides, &x3d, x3d_strides, in_dtype, &cam_mats, cam_batch, &ransac_thr, B, P,
                              istd_thres, flags, max_iters, &init_pose, &init_mask, &init_valid, &diag, debug_hypotheses, workspace, workspace_bytes, stream);
}

size_t mr_epnp_workspace_bytes(int B, int P) {
    if (B <= 0 || P < 4) return 0;
    return epnp_work_bytes(B, P, nullptr, nullptr);
}

int mr_epnp_ransac_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *ransac_thr, int B, int P,
    float istd_thres, int flags, int max_iters,
    double *const *init_pose, uint8_t *const *init_mask, uint8_t *const *init_valid, float *const *diag,
    void *workspace, size_t workspace_bytes, void *stream) {
    return epnp_ransac_launch(ncalls, x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, in_dtype, cam_mats, cam_batch, ransac_thr, B, P,
                              istd_thres, flags, max_iters, init_pose, init_mask, init_valid, diag, nullptr, workspace, workspace_bytes, stream);
}

int mr_pnp_uncert_from_init_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const double *init_pose, const uint8_t *init_mask, const uint8_t *init_valid, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *valid, float *pose, float *cov, float *tr_radius, uint8_t *inlier_mask, float *diag, void *stream) {
    if (B > 0 && (!init_pose || !init_mask || !init_valid)) return MR_ERR_BAD_ARGUMENT;
    return pnp_uncert_launch({ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch }, in_dtype,
                             nullptr, init_pose, init_mask, init_valid, B, P, z_min, 0.0f, inlier_opt_only, flags,
                             valid, pose, cov, tr_radius, inlier_mask, diag, stream);
}

static int pnp_from_init_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *u_range, const float *const *v_range, int range_batch,
    const double *const *init_pose, const uint8_t *const *init_mask, const uint8_t *const *init_valid, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *const *valid, float *const *pose, float *const *cov, float *const *tr_radius, uint8_t *const *inlier_mask, float *const *diag, void *stream,
    EpnpRefitIn *rf = nullptr, float *const *epnp_diag = nullptr, const float *calib_logscale = nullptr, float corr_sd = 0.0f, float *const *cov_calib = nullptr) {
    if (ncalls < 1 || ncalls > 8 || B < 0) return MR_ERR_BAD_ARGUMENT;
    const bool with_calib = cov_calib && cov_calib[0];
    if (with_calib && (!calib_logscale || (flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!x2d || !istd || !x3d || !x2d_strides || !istd_strides || !x3d_strides || !cam_mats || !u_range || !v_range || !init_pose || !init_mask || !init_valid ||
        !valid || !pose || !tr_radius || (!cov && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;       // (no covariance asked: the table itself may be NULL, like its entries)
    if ((long long)B * ncalls > 0x7fffffffll / kEpMaxIters) return MR_ERR_UNSUPPORTED;                         // objects are numbered through the set in int arithmetic (as in epnp_ransac_launch)
    const long long ks = (cam_batch == 1) ? 0 : 9, rs = (range_batch == 1) ? 0 : 2;
    PnpCallTable::CallPtrs cp[8];
    for (int c = 0; c < ncalls; ++c) {
        if (!x2d[c] || !istd[c] || !x3d[c] || !cam_mats[c] || !u_range[c] || !v_range[c] || !init_pose[c] || !init_mask[c] || !init_valid[c] ||
            !valid[c] || !pose[c] || !tr_radius[c] || (!(cov && cov[c]) && !(flags & MR_COV_NONE))) return MR_ERR_BAD_ARGUMENT;
        const CallBias at(c, B, in_dtype);
        if (at.mixed(inlier_mask) || at.mixed(diag) || at.mixed(cov_calib)) return MR_ERR_BAD_ARGUMENT;       // all or none
        PnpCallTable::CallPtrs &q = cp[c];
        q.x2d = at(x2d, x2d_strides); q.istd = at(istd, istd_strides); q.x3d = at(x3d, x3d_strides);
        q.K = at(cam_mats, ks); q.ur = at(u_range, rs); q.vr = at(v_range, rs);
        q.init_pose = at(init_pose, 4); q.init_mask = at(init_mask, P); q.init_valid = at(init_valid, 1);
        q.valid = at(valid, 1); q.pose = at(pose, 4); q.cov = at(cov, 16); q.tr = at(tr_radius, 1);
        q.mask = at(inlier_mask, P); q.diag = at(diag, 4); q.cov_calib = at(cov_calib, 16);
        if (rf) rf->diag[c] = at(epnp_diag, 4);
    }
    return pnp_uncert_launch({ x2d[0], x2d_strides, istd[0], istd_strides, x3d[0], x3d_strides, cam_mats[0], cam_batch, u_range[0], v_range[0], range_batch },
                             in_dtype, nullptr, init_pose[0], init_mask[0], init_valid[0], B, P, z_min, 0.0f, inlier_opt_only, flags,
                             valid[0], pose[0], cov ? cov[0] : nullptr, tr_radius[0], inlier_mask ? inlier_mask[0] : nullptr, diag ? diag[0] : nullptr, stream,
                             ncalls, cp, rf, calib_logscale, corr_sd);
}

int mr_pnp_uncert_from_init_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *u_range, const float *const *v_range, int range_batch,
    const double *const *init_pose, const uint8_t *const *init_mask, const uint8_t *const *init_valid, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *const *valid, float *const *pose, float *const *cov, float *const *tr_radius, uint8_t *const *inlier_mask, float *const *diag, void *stream) {
    return pnp_from_init_grouped(ncalls, x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, in_dtype, cam_mats, cam_batch, u_range, v_range, range_batch,
                                 init_pose, init_mask, init_valid, B, P, z_min, inlier_opt_only, flags, valid, pose, cov, tr_radius, inlier_mask, diag, stream);
}

int mr_pnp_uncert_from_epnp_grouped(
    int ncalls, const void *const *x2d, const int64_t *x2d_strides, const void *const *istd, const int64_t *istd_strides,
    const void *const *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *const *cam_mats, int cam_batch, const float *const *u_range, const float *const *v_range, int range_batch,
    double *const *init_pose, const uint8_t *const *init_mask, uint8_t *const *init_valid, float *const *epnp_diag, int B, int P,
    float z_min, int inlier_opt_only, int flags,
    uint8_t *const *valid, float *const *pose, float *const *cov, float *const *tr_radius, uint8_t *const *inlier_mask, float *const *diag,
    const float *cov_calib_logscale, float cov_corr_sd, float *const *cov_calib,
    const void *workspace, size_t workspace_bytes, void *stream) {
    if (ncalls < 1 || ncalls > kEpMaxGroup || B < 0 || P < 4) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if ((long long)B * ncalls > 0x7fffffffll / kEpMaxIters) return MR_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < epnp_work_bytes(B * ncalls, P, nullptr, nullptr)) return MR_ERR_BAD_ARGUMENT;
    EpnpRefitIn rf;
    memset(&rf, 0, sizeof rf);
    epnp_work_bytes(B * ncalls, P, &rf.w, (unsigned char *)const_cast<void *>(workspace));
    rf.B = (long long)B * ncalls;
    return pnp_from_init_grouped(ncalls, x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, in_dtype, cam_mats, cam_batch, u_range, v_range, range_batch,
                                 (const double *const *)init_pose, init_mask, (const uint8_t *const *)init_valid, B, P, z_min, inlier_opt_only, flags,
                                 valid, pose, cov, tr_radius, inlier_mask, diag, stream, &rf, epnp_diag, cov_calib_logscale, cov_corr_sd, cov_calib);
}

int mr_cov_symeig_rule(uint8_t *valid, float *cov, int B, float *eig_min_max, void *stream) {
    if (B < 0) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!valid || !cov) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(cov_symeig_rule_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, valid, cov, B, eig_min_max);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

int mr_pnp6_refine_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const uint8_t *inlier_mask, const float *pose4, const uint8_t *valid4, int B, int P, float z_min, int flags,
    uint8_t *valid, float *pose6, float *cov6, float *diag, void *stream) {
    const CorrIn in{ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (B < 0 || P < 4 || P > 64 * kMaxChunks) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !inlier_mask || !pose4 || !valid4 || !valid || !pose6 || !cov6) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    Pnp6Args a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.mask = inlier_mask; a.pose4 = pose4; a.valid4 = valid4;
    a.B = B; a.P = P; a.z_min = (double)z_min; a.lm_max_iter = lm_max_iter(flags);
    a.valid = valid; a.pose6 = pose6; a.cov6 = cov6; a.diag = diag;
    return with_storage_type(in_dtype, [&](auto t) { return launch_pnp6<typename decltype(t)::type>(a, (hipStream_t)stream); });
}

int mr_pnp_exact_hessian_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const float *pose, const uint8_t *inlier_mask, int B, int P, float z_min,
    uint8_t *valid, float *hess, float *cov, void *stream) {
    const CorrIn in{ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (B < 0 || P < 1) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !pose || !valid || !cov) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    HessArgs a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.pose = pose; a.mask = inlier_mask; a.B = B; a.P = P; a.z_min = (double)z_min;
    a.valid = valid; a.hess = hess; a.cov = cov;
    return with_storage_type(in_dtype, [&](auto t) {
        hipLaunchKernelGGL((exact_hessian_kernel<typename decltype(t)::type>), dim3(B), dim3(256), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    });
}

int mr_pnp_uncert_backward_batched(
    const void *x2d, const int64_t *x2d_strides, const void *istd, const int64_t *istd_strides,
    const void *x3d, const int64_t *x3d_strides, int in_dtype,
    const float *cam_mats, int cam_batch, const float *u_range, const float *v_range, int range_batch,
    const float *pose, const uint8_t *inlier_mask, const uint8_t *valid, int lm_all_points,
    const float *grad_pose, const float *cov, const float *grad_cov, int B, int P, float z_min,
    float *grad_x2d, float *grad_istd, float *grad_x3d, uint8_t *status, void *stream) {
    const CorrIn in{ x2d, x2d_strides, istd, istd_strides, x3d, x3d_strides, cam_mats, cam_batch, u_range, v_range, range_batch };
    if (B < 0 || P < 1) return MR_ERR_BAD_ARGUMENT;
    if (B == 0) return MR_OK;
    if (!in.complete() || !pose || !valid) return MR_ERR_BAD_ARGUMENT;
    if ((cov == nullptr) != (grad_cov == nullptr)) return MR_ERR_BAD_ARGUMENT;
    if (!in.batches_ok(B)) return MR_ERR_BAD_ARGUMENT;
    PnpBwdArgs a;
    memset(&a, 0, sizeof a);
    set_inputs(a, in);
    a.pose = pose; a.mask = inlier_mask; a.valid = valid; a.lm_all = lm_all_points ? 1 : 0;
    a.grad_pose = grad_pose; a.cov = cov; a.grad_cov = grad_cov;
    a.B = B; a.P = P; a.z_min = (double)z_min;
    a.g2 = grad_x2d; a.gw = grad_istd; a.g3 = grad_x3d; a.status = status;
    return with_storage_type(in_dtype, [&](auto t) {
        hipLaunchKernelGGL((pnp_uncert_backward_kernel<typename decltype(t)::type>), dim3(B), dim3(256), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    });
}
