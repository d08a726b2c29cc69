// host_launch.inc — the host side of the launches (included by monorun_pnp.hip inside its anonymous namespace, after every kernel): the LDS
// carve, the summation-plan builder, the per-device state, the LDS grant, the launchers and what the C ABI uses to fill their arguments.
size_t lds_bytes(const PnpArgs &a, int wpo) {
    size_t n = 0;
    n += sizeof(double) * (2 * wpo * kRedN + kMsg);       // reduction scratch + leader/follower message + camera matrix
    n += sizeof(unsigned long long) * a.nca;
    n += sizeof(float) * kHyp * 8;
    n += sizeof(int) * wpo * kHyp;
    n += sizeof(float) * (4 * a.nla + 4);
    const bool small = wpo <= 2;                           // one- and two-wave instantiations: 12-byte B records at fp32, one index list (pnp_kernel.inc)
    n += (size_t)((small && a.elem_size == 4) ? 7 : 8) * a.P * a.elem_size;      // point records
    n += (small ? 1 : 2) * sizeof(uint16_t) * ((a.P + 7) & ~7);                   // candidate list (+ final inlier list)
    n += small ? sizeof(unsigned long long) * a.nca + 8 : (size_t)a.P;           // inlier mask: one bit (64-bit words on an 8-byte boundary: up to 4 bytes of padding) or one byte per point
    return (n + 15) & ~(size_t)15;
}

struct PlanNode { int left, right, height; };

int plan_rec(PairwisePlan &pl, std::vector<PlanNode> &nodes, int off, int n, bool &ok) {
    if (n <= 128) {                                     // numpy: n < 8 plain loop, n <= PW_BLOCKSIZE unrolled block
        if (pl.n_leaves >= kMaxLeaves) { ok = false; return 0; }
        pl.leaf_off[pl.n_leaves] = (uint16_t)off; pl.leaf_len[pl.n_leaves] = (uint16_t)n;
        return pl.n_leaves++;                           // slot of a leaf = its index
    }
    int n2 = n / 2; n2 -= n2 % 8;
    const int l = plan_rec(pl, nodes, off, n2, ok); if (!ok) return 0;
    const int r = plan_rec(pl, nodes, off + n2, n - n2, ok); if (!ok) return 0;
    auto height = [&](int s) { return s < 0 ? nodes[-s - 1].height : 0; };
    nodes.push_back({ l, r, 1 + (height(l) > height(r) ? height(l) : height(r)) });
    return -(int)nodes.size();                          // internal nodes: negative ids until renumbered
}

bool build_plan(PairwisePlan &pl, int P) {
    memset(&pl, 0, sizeof pl);
    std::vector<PlanNode> nodes;
    bool ok = true;
    const int root = plan_rec(pl, nodes, 0, P, ok);
    if (!ok || nodes.size() > (size_t)kMaxLeaves) return false;
    // order internal nodes by height (stable), renumber
    std::vector<int> order(nodes.size()), newid(nodes.size());
    int maxh = 0;
    for (auto &nd : nodes) if (nd.height > maxh) maxh = nd.height;
    if (maxh + 1 >= 16) return false;
    int k = 0;
    for (int h = 1; h <= maxh; ++h) {
        pl.level_start[h - 1] = (uint8_t)k;
        for (size_t i = 0; i < nodes.size(); ++i) if (nodes[i].height == h) { order[k] = (int)i; newid[i] = k; ++k; }
    }
    pl.level_start[maxh] = (uint8_t)k;
    pl.n_levels = maxh; pl.n_internal = (int)nodes.size();
    auto slot = [&](int s) { return s >= 0 ? s : pl.n_leaves + newid[-s - 1]; };
    for (int i = 0; i < pl.n_internal; ++i) { pl.left[i] = (uint8_t)slot(nodes[order[i]].left); pl.right[i] = (uint8_t)slot(nodes[order[i]].right); }
    pl.root = slot(root);
    return true;
}

std::atomic<int> g_last_hip_error{0};
unsigned long long *g_stamps = nullptr;
#ifdef MR_DEBUG_STAMPS
unsigned long long *g_cons_stamps = nullptr;
#endif
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { g_last_hip_error = (int)e_; return MR_ERR_HIP; } } while (0)

// What the heuristics below need to know about the device, read once per device from hipGetDeviceProperties (an MI355X reports
// 256 CUs and 160 KB of LDS per CU; a partitioned or future part reports its own).  CDNA compute units have 4 SIMDs.
struct DevInfo { int cus; size_t lds_per_cu; };
DevInfo dev_info() {
    static std::mutex mu; static DevInfo cache[kMaxDevices]; static bool have[kMaxDevices] = {};
    int dev = 0;
    DevInfo d = { 256, (size_t)160 * 1024 };
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return d;
    std::lock_guard<std::mutex> lk(mu);
    if (!have[dev]) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) == hipSuccess) {
            if (pr.multiProcessorCount > 0) d.cus = pr.multiProcessorCount;
            if (pr.maxSharedMemoryPerMultiProcessor > 0) d.lds_per_cu = pr.maxSharedMemoryPerMultiProcessor;
        }
        cache[dev] = d; have[dev] = true;
    }
    return cache[dev];
}
constexpr int kSimdsPerCu = 4;

// The grid of a 1-D launch over `total` items, `per_block` to a workgroup: MR_ERR_UNSUPPORTED beyond the 2^31 - 1 workgroups of a grid dimension
int grid_1d(long long total, int per_block, unsigned &blocks) {
    const long long n = (total + per_block - 1) / per_block;
    blocks = (unsigned)n;
    return n > 0x7fffffffLL ? MR_ERR_UNSUPPORTED : MR_OK;
}

// Opts a kernel in to more dynamic LDS than the default 48 KB.  The grant is a per-device function attribute, kept per (kernel, device):
// raised monotonically and under a lock (two host threads with different sizes must not shrink it between the other's set and launch),
// and no driver call in the steady state.  Launches within the default take neither the lock nor the attribute.
int grant_lds(const void *fn, size_t lds) {
    if (lds <= 48 * 1024) return MR_OK;
    static std::mutex mu; static std::map<std::pair<const void *, int>, size_t> granted;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    size_t &g = granted[std::make_pair(fn, dev)];
    if (lds > g) {
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        g = lds;
    }
    return MR_OK;
}

// One launch of an LM kernel: a workgroup of WPO waves per object, the LDS lds_bytes() carves, `a` and then `more` as the kernel's arguments.
// any_order (MR_ANY_ORDER, for the kernels that honour it): no barrier bit on the dispatch packet — the launch starts once the launch in front of
// it has STARTED (the LM launches of the calls of one launch set: the first waits for the set's initialiser launches, the others run beside it —
// PnPEpnpGroupLaunch).
template <int WPO, typename Kernel, typename... More>
int launch_lm(Kernel kernel, bool any_order, const PnpArgs &a, hipStream_t st, const More &... more) {
    const size_t lds = lds_bytes(a, WPO);
    if (lds > dev_info().lds_per_cu) return MR_ERR_UNSUPPORTED;
    int r;
    if ((r = grant_lds((const void *)kernel, lds)) != MR_OK) return r;
    if (any_order) hipExtLaunchKernelGGL(kernel, dim3(a.B), dim3(64 * WPO), (uint32_t)lds, st, nullptr, nullptr, hipExtAnyOrderLaunch, a, more...);
    else hipLaunchKernelGGL(kernel, dim3(a.B), dim3(64 * WPO), lds, st, a, more...);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// the fast mode's launch: the object's own initialiser (K0) inside the kernel
template <typename T, int WPO>
int launch(const PnpArgs &a, hipStream_t st) { return launch_lm<WPO>(pnp_uncert_kernel<T, WPO>, a.flags & MR_ANY_ORDER, a, st); }

// behind an external initialiser: with the initialiser's re-fit as the launch's prologue (rf: mr_pnp_uncert_from_epnp_grouped; always with a
// call table), over the objects of several calls (tbl: the kernel that takes the call table as a second argument), or over one call's objects
template <typename T, int WPO>
int launch_ext(const PnpArgs &a, hipStream_t st, const PnpCallTable *tbl, const EpnpRefitIn *rf) {
    if (rf) return launch_lm<WPO>(pnp_uncert_refit_kernel<T, WPO>, false, a, st, *tbl, *rf);
    if (tbl) return launch_lm<WPO>(pnp_uncert_group_kernel<T, WPO>, false, a, st, *tbl);
    return launch_lm<WPO>(pnp_uncert_kernel<T, WPO, true>, a.flags & MR_ANY_ORDER, a, st);
}

// the instantiations of the external-initialiser launch (launch_ext): 2, 4 or 8 waves per object
int ext_wpo(int wpo) { return wpo < 2 ? 2 : (wpo == 3 ? 4 : wpo); }

// What a launch derives from its arguments: the storage size, the coalesced per-point loads (channel-planar rows: point stride 1 on all three
// tensors; never from_head, whose tile is decoded in-kernel) and, for PnpArgs, the LDS carve: chunk slots (multiple of 4), pairwise leaves (>= 1).
template <typename T, class A>
void derive_launch_fields(A &a) {
    a.elem_size = (int)sizeof(T);
    a.vec = (!a.from_head && a.s2[1] == 1 && a.sw[1] == 1 && a.s3[1] == 1) ? 1 : 0;
    if constexpr (std::is_same<A, PnpArgs>::value) {
        a.nca = (((a.P + 63) / 64) + 3) & ~3;
        a.nla = a.plan.n_leaves > 0 ? a.plan.n_leaves : 1;
    }
}

// Ceres' max_num_iterations: 50 unless the MR_LM_MAXIT bits of `flags` are set
int lm_max_iter(int flags) {
    const int mi = (flags & MR_LM_MAXIT_MASK) >> MR_LM_MAXIT_SHIFT;
    return mi ? mi : 50;
}

template <typename T>
int launch_wpo(PnpArgs &a, int wpo, hipStream_t st, const PnpCallTable *tbl = nullptr, const EpnpRefitIn *rf = nullptr) {
    derive_launch_fields<T>(a);
    a.lm_max_iter = lm_max_iter(a.flags);
    if (a.init_mask) {                      // external initialiser: 2, 4 or 8 waves per object
        switch (ext_wpo(wpo)) {
            case 2: return launch_ext<T, 2>(a, st, tbl, rf);
            case 4: return launch_ext<T, 4>(a, st, tbl, rf);
            case 8: return launch_ext<T, 8>(a, st, tbl, rf);
            default: return MR_ERR_BAD_ARGUMENT;
        }
    }
    if (tbl) return MR_ERR_BAD_ARGUMENT;
    switch (wpo) {
        case 1: return launch<T, 1>(a, st);
        case 2: return launch<T, 2>(a, st);
        case 3: return launch<T, 3>(a, st);
        case 4: return launch<T, 4>(a, st);
        case 8: return launch<T, 8>(a, st);
        default: return MR_ERR_BAD_ARGUMENT;
    }
}

int pick_wpo(int B, int P, int flags) {
    int w = (flags & MR_WAVES_MASK) >> MR_WAVES_SHIFT;
    if (w) return w;
    // fp32 variants hold 4 resident waves per SIMD (<= 128 VGPRs) -> 4096 waves on 256 CUs x 4 SIMDs.  More waves per
    // object shorten an object's latency chain (what bounds small batches), fewer waves cost fewer instructions per object
    // (what bounds large ones).  Measured on MI355X, P = 784: 4 waves/object wins up to B = 2048, 2 from B = 4096
    // (i.e. while B x waves x 2 does not exceed twice the resident-wave capacity of the chip).
    const long long wave_slots = (long long)dev_info().cus * kSimdsPerCu * 4;      // 4096 on an MI355X
    w = 1;
    while (w < 4 && (long long)B * w * 2 <= 2 * wave_slots && P >= 64 * w * 2) w *= 2;      // small batches: fill the SIMDs
    int wp = 1;
    while (wp < 4 && P > 64 * wp * 8) wp *= 2;                                     // large tiles: <= ~8 points per lane
    if (wp > w) w = wp;                                                            // (P = 784 -> 2, P = 3136 -> 4)
    return w;
}

// Tiles so large that at most two workgroups fit the LDS of a CU (config 5: 56x56 points, 66 KB as fp16, 100 KB as fp32 against 160 KB):
// with 4 waves per object a CU would hold 8 waves; 8 waves per object restore 16 (4 per SIMD — the 128-VGPR kernels allow it).
// Measured on the config-5 shard (8192 objects, fp16): 0.851 -> 0.810 ms.
int widen_for_large_tiles(int wpo, const PnpArgs &a, int flags, int in_dtype) {
    if ((flags & MR_WAVES_MASK) || wpo != 4 || in_dtype == MR_F64 || a.P < 64 * 8 * 2) return wpo;
    PnpArgs t = a;
    t.elem_size = (in_dtype == MR_F16) ? 2 : 4;                 // the launcher sets it later, from the template type
    return (lds_bytes(t, 4) * 3 > dev_info().lds_per_cu) ? 8 : wpo;
}

// Waves per object of the LM / covariance launch of pnp_uncert_launch: the size rule, widened for large tiles, and with an external
// initialiser (a.init_mask: the default flow) the nearest instantiation launch_ext has.  The covariance stage's summation tree follows
// this count; mr_debug_launch_waves answers with this same function, so what the tests ask for is what the launch uses.
int lm_launch_waves(const PnpArgs &a, int flags, int in_dtype) {
    const int w = widen_for_large_tiles(pick_wpo(a.B, a.P, flags), a, flags, in_dtype);
    return a.init_mask ? ext_wpo(w) : w;
}

// development aid for the tests (mr_debug_block_sum): block_sum_packed<WPO, 10> — the covariance stage's reduction — on caller-supplied
// per-lane partials (64 WPO lanes x 10), one workgroup; lanes 0..9 of every wave write their totals to out[wave * 10 + k]
template <int WPO>
__global__ void __launch_bounds__(64 * WPO) block_sum_probe_kernel(const double *part, double *out) {
    __shared__ double red[2 * WPO * kRedN];
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = part[threadIdx.x * 10 + k];
    int flip = 0;
    const double t = block_sum_packed<WPO, 10>(acc, red, flip);
    const int lane = threadIdx.x & 63;
    if (lane < 10) out[(threadIdx.x >> 6) * 10 + lane] = t;
}

// 6-DoF refinement (second launch of pnp_uncert(..., use_6dof=True)): see pnp6_kernel.inc
template <typename T>
int launch_pnp6(Pnp6Args &a, hipStream_t st) {
    derive_launch_fields<T>(a);
    const int nchunk = (a.P + 63) / 64;
    const size_t lds = sizeof(double) * 2 * 4 * kRedN + sizeof(unsigned long long) * ((nchunk + 3) & ~3) + (size_t)8 * a.P * sizeof(T) +
                       sizeof(uint16_t) * ((a.P + 7) & ~7) + 16;
    if (lds > dev_info().lds_per_cu) return MR_ERR_UNSUPPORTED;
    int r;
    if ((r = grant_lds((const void *)pnp6_refine_kernel<T>, lds)) != MR_OK) return r;
    hipLaunchKernelGGL((pnp6_refine_kernel<T>), dim3(a.B), dim3(kThreads6), lds, st, a);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// One launch of a lane-mapped kernel (epnp_stages.inc) at its level, over `items` matrices: a wave per item (level 4), a 16-lane row (2) or
// a quad (0), in single-wave workgroups
template <typename Kernel>
void launch_lane_mapped(Kernel wave, Kernel row, Kernel quad, int level, long long items, hipStream_t st, const EpnpStageArgs &ea) {
    const int per_wave = level == 4 ? 1 : (level == 2 ? 4 : 16);
    hipLaunchKernelGGL(level == 4 ? wave : (level == 2 ? row : quad), dim3((unsigned)((items + per_wave - 1) / per_wave)), dim3(64), 0, st, ea);
}

// The staged form of the initialiser (epnp_stages.inc): six or seven launches on `st` (the second round idles when no object needs it: one launch for small sets, two beyond), intermediate results in `workspace` (caller's, at
// least mr_epnp_workspace_bytes(B, P)) or, when that is null, in a stream-ordered allocation of the device's default memory pool.
template <typename T>
int launch_epnp_stages(EpnpStageArgs &ea, void *workspace, size_t workspace_bytes, int first_round, hipStream_t st) {
    PnpArgs &a = ea.p;
    derive_launch_fields<T>(a);
    const size_t lds_f = epnp_front_lds_bytes(a), lds_c = epnp_consensus_lds_bytes(a), lds_r = epnp_refit_lds_bytes(a);
    if (lds_f > dev_info().lds_per_cu || lds_c > dev_info().lds_per_cu || lds_r > dev_info().lds_per_cu) return MR_ERR_UNSUPPORTED;
    const size_t need = epnp_work_bytes(a.B, a.P, nullptr, nullptr);
    unsigned char *base = (unsigned char *)workspace;
    bool own = false;
    if (base) { if (workspace_bytes < need || ((uintptr_t)base & 255)) return MR_ERR_BAD_ARGUMENT; }
    else {
        // a PRIVATE stream-ordered pool per device (the process's default pool is left as it is): freed workspaces stay in it across
        // synchronisations (release threshold = max), so the steady state allocates nothing
        static std::mutex mu; static hipMemPool_t pools[kMaxDevices] = {};
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (dev < 0 || dev >= kMaxDevices) return MR_ERR_UNSUPPORTED;
        hipMemPool_t pool;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (!pools[dev]) {
                hipMemPoolProps props;
                memset(&props, 0, sizeof props);
                props.allocType = hipMemAllocationTypePinned;
                props.handleTypes = hipMemHandleTypeNone;
                props.location.type = hipMemLocationTypeDevice;
                props.location.id = dev;
                HIP_TRY(hipMemPoolCreate(&pools[dev], &props));
                uint64_t keep = ~0ull;
                HIP_TRY(hipMemPoolSetAttribute(pools[dev], hipMemPoolAttrReleaseThreshold, &keep));
            }
            pool = pools[dev];
        }
        HIP_TRY(hipMallocFromPoolAsync((void **)&base, need, pool, st));
        own = true;
    }
    epnp_work_bytes(a.B, a.P, &ea.w, base);
    int rc = MR_OK;
    auto run = [&]() -> int {
        int r;
        if ((r = grant_lds((const void *)epnp_front_kernel<T>, lds_f)) != MR_OK) return r;
        if ((r = grant_lds((const void *)epnp_consensus_kernel<T, 4>, lds_c)) != MR_OK) return r;
        if ((r = grant_lds((const void *)epnp_refit_kernel<T>, lds_r)) != MR_OK) return r;
        // The 30 hypotheses of an object are solved in two rounds: [0, first) for every object, the rest only for the objects whose
        // replayed loop still wants iterations after `first` (ptsetreg.cpp's adaptive bound: with few outliers it drops to a
        // handful after the first good model — config-2 batches: 1.5 iterations on average, 8 at most).  Same results either way.
        const int first = first_round < 1 ? 1 : (first_round > kEpMaxIters ? kEpMaxIters : first_round);
        ea.h0 = 0; ea.h1 = first;                             // the front launch fetches the samples of the first round only
        hipLaunchKernelGGL((epnp_front_kernel<T>), dim3(a.B), dim3(kEpThreads), lds_f, st, ea);
        // small launch sets (one call at a time): the second round as ONE launch (epnp_round2_kernel); launch sets in flight keep the two compact ones
        // development / tests: force the quads per matrix (0, 2 or 4 levels) of both lane-mapped launches (MR_EP_WIDE) or of one (MR_EP_WIDE_HYP, MR_EP_WIDE_BETAS)
        static const auto lv_env = [](const char *name) { const char *e = getenv(name); const int v = e ? atoi(e) : -1; return (v == 0 || v == 2 || v == 4) ? v : -1; };
        static const int wide_env = lv_env("MR_EP_WIDE");
        static const int wide_hyp_env = lv_env("MR_EP_WIDE_HYP") >= 0 ? lv_env("MR_EP_WIDE_HYP") : wide_env, wide_betas_env = lv_env("MR_EP_WIDE_BETAS") >= 0 ? lv_env("MR_EP_WIDE_BETAS") : wide_env;
        static const int r2_env = [] { const char *e = getenv("MR_EP_ROUND2"); return e ? atoi(e) : 0; }();      // development: 1 = always two launches, 2 = always one
        const bool one_launch_round2 = (kEpMaxIters - first) <= kEpRound2Quads && first < kEpMaxIters && (r2_env == 2 || (r2_env == 0 && a.B < 2048));
        for (int round = 0; round < 2; ++round) {
            ea.h0 = round == 0 ? 0 : first; ea.h1 = round == 0 ? first : kEpMaxIters;
            const int nh = ea.h1 - ea.h0;
            if (nh <= 0) break;
            if (round == 1 && one_launch_round2) {
                const size_t lds_2 = epnp_round2_lds_bytes(a);
                if ((r = grant_lds((const void *)epnp_round2_kernel<T>, lds_2)) != MR_OK) return r;
                hipLaunchKernelGGL((epnp_round2_kernel<T>), dim3(a.B), dim3(256), lds_2, st, ea);
                break;
            }
            const long long quads = (long long)a.B * nh;
            // 16 quads per single-wave workgroup: 8 / 4 per wave (more waves, fewer matrices in lockstep) measured 74 / 140 us against 74 us one call
            // at a time and 5.4 / 4.1 against 6.3 M solves/s in flight (profiles/r04_epnp_quads_per_wave.txt)
            // wide form (a wave per hypothesis) while that still leaves SIMDs without a wave: up to 1024 hypotheses (one image's <= 100 proposals x the first
            // round of 10).  Measured, one call at a time (profiles/r06_wide_sweep.txt): B = 100: -6 us; a 16-lane row per hypothesis at B = 200 / 320: +-0; a wave
            // at B = 200: +40 us (2000 waves: the chip is full and its clock drops)
            const int lv_h = wide_hyp_env >= 0 ? wide_hyp_env : (quads <= 1024 ? 4 : (quads <= 4096 ? 2 : 0));      // (rows up to 4096 hypotheses: B = 128 ... 400: -9 ... -3 us; 5120: +30)
            launch_lane_mapped(epnp_hyp_kernel<4>, epnp_hyp_kernel<2>, epnp_hyp_kernel<0>, lv_h, quads, st, ea);
            hipLaunchKernelGGL((epnp_consensus_kernel<T, 4>), dim3(a.B), dim3(256), lds_c, st, ea);      // 4 waves per object (epnp_stages.inc)
        }
        {   // (quad form with 8 / 4 / 2 quads per wave: 67 / 68 / 102 us against 55 us, round 4)
            // a wave per object up to 512 objects, a 16-lane row up to 2047 (B = 100: -10 us, 512: -5, 1024: -5 with rows, +16 with waves), the quad form for launch sets
            const int lv_b = wide_betas_env >= 0 ? wide_betas_env : (a.B <= 512 ? 4 : (a.B < 2048 ? 2 : 0));
            launch_lane_mapped(epnp_refit_betas_kernel<4>, epnp_refit_betas_kernel<2>, epnp_refit_betas_kernel<0>, lv_b, a.B, st, ea);
        }
        if (!(a.flags & MR_EPNP_DEFER_REFIT))                  // else: the LM launch carries it (mr_pnp_uncert_from_epnp_grouped)
            hipLaunchKernelGGL((epnp_refit_kernel<T>), dim3(a.B), dim3(kEpPoseThreads), lds_r, st, ea);
        HIP_TRY(hipGetLastError());
        return MR_OK;
    };
    rc = run();
    if (own) { const hipError_t e = hipFreeAsync(base, st); if (rc == MR_OK && e != hipSuccess) { g_last_hip_error = (int)e; rc = MR_ERR_HIP; } }
    return rc;
}

// N8, the training decode (noc_decode_train_kernel.inc): the forward with a thread per RoI pixel, (h w + 255) / 256 workgroups per object as the
// scalar K2 kernel; the backward with a workgroup per object
int launch_noc_decode_train(const DecodeTrainArgs &t, hipStream_t st) {
    unsigned blocks;
    if (grid_1d((long long)((t.d.h * t.d.w + 255) / 256) * t.d.B, 1, blocks) != MR_OK) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(noc_decode_train_kernel, dim3(blocks), dim3(256), 0, st, t);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}
int launch_noc_decode_train_backward(const DecodeTrainArgs &t, hipStream_t st) {
    hipLaunchKernelGGL(noc_decode_train_backward_kernel, dim3((unsigned)t.d.B), dim3(256), 0, st, t);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// The correspondence inputs of the per-object launches as the C ABI passes them: x2d / istd / x3d with their (b, p, c) element strides, the
// fp32 camera matrices and u / v clip ranges (a batch of 1 is broadcast to every object).
struct CorrIn {
    const void *x2d; const int64_t *s2; const void *istd; const int64_t *sw; const void *x3d; const int64_t *s3;
    const float *K; int cam_batch; const float *ur, *vr; int range_batch;
    bool complete() const { return x2d && s2 && istd && sw && x3d && s3 && K && ur && vr; }
    bool batches_ok(int B) const { return (cam_batch == 1 || cam_batch == B) && (range_batch == 1 || range_batch == B); }
};
// ... copied into a kernel's argument struct (PnpArgs, Pnp6Args, HessArgs, PnpBwdArgs: the same field names, each struct its own layout)
template <class A>
void set_inputs(A &a, const CorrIn &in) {
    a.x2d = in.x2d; a.istd = in.istd; a.x3d = in.x3d;
    for (int i = 0; i < 3; ++i) { a.s2[i] = in.s2[i]; a.sw[i] = in.sw[i]; a.s3[i] = in.s3[i]; }
    a.K = in.K; a.K_stride = (in.cam_batch == 1) ? 0 : 9;
    a.ur = in.ur; a.vr = in.vr; a.r_stride = (in.range_batch == 1) ? 0 : 2;
}

// The order of the istd means (MR_MEAN_* bits of a.flags; AUTO: numpy's pairwise tree where the istd rows are contiguous, always for from_head,
// whose tile is channel-planar) and the tree's plan where the kernel forms the means itself (no external initialiser's mask).
int choose_mean_order(PnpArgs &a) {
    int mm = a.flags & MR_MEAN_MASK;
    if (mm == MR_MEAN_AUTO) mm = (a.from_head || (a.sw[1] == 1 && a.P > 1)) ? MR_MEAN_PAIRWISE : MR_MEAN_SEQUENTIAL;
    a.mean_mode = mm;
    if (mm == MR_MEAN_PAIRWISE && !(a.flags & MR_NO_ISTD_MASK) && !a.init_mask && !build_plan(a.plan, a.P)) return MR_ERR_UNSUPPORTED;
    return MR_OK;
}

// Grouped launches run the objects of several calls of B objects each as one batch: object i of call c is object c * B + i, and call c's pointers
// are biased so that this GLOBAL index addresses them (EpnpCallPtrs, PnpCallTable::CallPtrs).  Optional per-call pointers (a table that may be
// NULL, entries that may be NULL) are given for all calls or for none.
struct CallBias {
    int c; long long o, esize;              // the call, its first object in the batch, bytes per element of the correspondence tensors
    CallBias(int call, int B, int in_dtype) : c(call), o((long long)call * B), esize(in_dtype == MR_F64 ? 8 : (in_dtype == MR_F32 ? 4 : 2)) {}
    // a correspondence tensor: strides[0] elements per object
    const void *operator()(const void *const *t, const int64_t *strides) const { return (const char *)t[c] - o * strides[0] * esize; }
    // any other pointer, `rows` elements per object (NULL stays NULL)
    template <typename P> P *operator()(P *const *t, long long rows) const { P *const q = t ? t[c] : nullptr; return q ? q - o * rows : nullptr; }
    // an optional pointer given for this call and not for call 0, or the other way round
    template <typename P> bool mixed(P *const *t) const { return (t && t[c]) != (t && t[0]); }
};

// f(TypeTag<T>{}) for the storage type of the correspondence tensors: float, __half or double
template <typename T> struct TypeTag { using type = T; };
template <typename F>
int with_storage_type(int in_dtype, F &&f) {
    switch (in_dtype) {
        case MR_F32: return f(TypeTag<float>{});
        case MR_F16: return f(TypeTag<__half>{});
        case MR_F64: return f(TypeTag<double>{});
        default: return MR_ERR_UNSUPPORTED;
    }
}
