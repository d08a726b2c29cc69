// epnp_stages.inc — the reference's initialiser (cv2.solvePnPRansac(iterationsCount = 30, flags = SOLVEPNP_EPNP),
// pnp_uncert_cpu.py:35-58) as a sequence of launches, each with the lanes-to-work mapping its stage wants.  The arithmetic is the
// specification of oracle/epnp.inc operation for operation (see the header of epnp_kernel.inc); only WHERE a value is computed
// differs from the one-kernel form this replaces (one workgroup per object for everything: 1.76 ms per 1024 objects, 256 VGPRs and
// 677 spills, two sequential eigen-solves of 250 us each with one active lane-group per workgroup).
//
//   front      one workgroup per object: records -> LDS, istd candidates (numpy's float32 summation order), the 30 five-point
//              subsets of cv::RNG((uint64)-1) (they do not depend on any model), their point indices and the first round's
//              samples' correspondences -> workspace
//   hyp        one QUAD per hypothesis of the round, everything in registers: control points, barycentric coordinates, M^T M (each lane
//              its rows), the four eigenvectors (epnp_eig_low4.inc), then lanes 0..2 = the beta candidates N = 1, 2, 3 on one code
//              path: approximation, Gauss-Newton, pose, reprojection error of each candidate -> workspace
//   consensus  one workgroup per object: the best candidate of every hypothesis through the Rodrigues round trip of solvePnP's
//              output, float32 reprojection test of all candidates against the round's hypotheses, OpenCV's
//              sequential loop replayed over the counts in RNG order, the winner's inlier mask / list, and the point sums of the
//              re-fit (centroid, PCA, M^T M); an object whose loop goes on: the correspondences of its second round's samples
//   refit_betas one quad per object: the re-fit's four eigenvectors, then lanes 0..2 = the beta candidates: the candidates' control
//              points in the camera frame, their pose (absolute orientation) and yaw
//   refit      one workgroup per object, one wave per candidate: reprojection error of each over the inliers (the waves'
//              butterflies), the best one's pose -> init_pose, init_ok, diag
// The speculative hypotheses are solved in TWO ROUNDS: [0, first) for every object, [first, 30) only for the objects whose replayed loop
// still wants iterations (the adaptive bound of RANSACUpdateNumIters drops to a handful after the first good model; the loop's state
// parks in the workspace between the rounds).  Where the split falls changes the work, never the result.
// Seven launches (round 3: thirteen); six for launch sets of fewer than 2048 objects, whose second round is ONE launch (epnp_round2_kernel).  Between the launches: a workspace laid out element-major ([element][problem]: a wave's accesses
// to one element of consecutive problems are contiguous), 12.0 MB per 1024 objects since round 15 (the re-fit's list as a bit row, 104 B per object at P = 784; round 8: 11.9 MB, round 5: 11.8 MB, round 4: 17 MB, round 3: 65 MB — the hypotheses' M^T M, control
// points, coordinates and eigenvectors no longer leave the registers).

constexpr int kEpMeta = 12;           // ints per object in the workspace
constexpr int kEpSampRec = 28;        // floats per sample record (25 used; seven 16-byte loads)
enum { EP_M_N = 0, EP_M_MODE, EP_M_NFIT, EP_M_REFIT, EP_M_ITERS, EP_M_BEST, EP_M_BESTH, EP_M_PENDING, EP_M_NITERS };
enum { EP_MODE_FAIL = 0, EP_MODE_PLAIN = 1, EP_MODE_RANSAC = 2 };
constexpr int kEpCandRec = 13;        // doubles per re-fit candidate record: R (9), t (3), yaw
constexpr int kEpCandStride = 40;     // doubles per object of the records (three, one pad)

struct EpnpWork {
    int *meta;            // [B][kEpMeta]: candidates, mode, points of the re-fit, re-fit wanted, iterations run, best count, best model,
                          //               second round wanted, the loop's current iteration bound
    float *samp;          // [NQ][28]: the five correspondences of every sample (X Y Z u v per point; 25 floats in a 112-byte record), NQ = 30 B;
                          //           the front launch writes the first round's, the consensus launch those a pending object's second round solves
    uint16_t *spt;        // [B][150]: the point index of every sample's five correspondences
    double *hrt;          // [12][NQ]: R (row-major, after the Rodrigues round trip) | t of every hypothesis' best beta candidate
    uint16_t *cand;       // [B][pstride] ascending candidate list
    uint16_t *fit;        // [B][pstride] the re-fit's point list
    double *prep_r;       // [B][24]: control points (12), inverse of the control-point basis (9).  The per-object results below are object-major: one
                          //          workgroup (one XCD's L2) writes an object's values, and they share cache lines with no other object's
    double *mtm_r;        // [B][144]
    double *cand_r;       // [B][kEpCandStride]: the re-fit's three candidate poses, kEpCandRec doubles each: R (row-major, 9), t (3), yaw = rvec[1]
    double *abt_r;        // [B][24]: the re-fit's absolute-orientation moments: sum a_j (4), sum a_j (pw - pw0) (4 x 3), sum (pw - pw0) (3), -, a(first inlier) (4)
    float *cam;           // [4][B]: fx fy cx cy of every object as the reference hands them to cv2 (float32), for the lane-mapped launches
    long long nq;
    int pstride;
};

// Several calls in ONE launch set (mr_epnp_ransac_grouped): HIP runs the launches of at most four streams side by side, and every stage of
// this initialiser is a latency chain that fills a fraction of the chip, so the way to have more than four calls' stages in flight is to
// let a launch carry the objects of several calls.  Objects are numbered through the group (b = g * group_B + local index), the
// workspace is laid out for all of them, and only the tensors a CALLER owns differ per call: their pointers, biased on the host so that
// the GLOBAL object index addresses them.  Strides, dtype, P, thresholds' presence and flags are common to the group.
constexpr int kEpMaxGroup = 8;
struct EpnpCallPtrs {
    const void *x2d, *istd, *x3d, *K;
    const float *ransac_thr;
    double *init_pose; uint8_t *init_mask; uint8_t *init_ok; float *diag;
};
struct EpnpStageArgs {
    PnpArgs p;              // correspondence tensors + strides, camera, RANSAC thresholds, istd-mask parameters (as for the LM kernel); p.B = ALL objects of the group
    EpnpWork w;
    int ncalls, group_B;    // calls in this launch set (1: p / init_* below are the call's own pointers) and objects per call
    EpnpCallPtrs call[kEpMaxGroup];
    double *init_pose;      // out (B,4) fp64 [yaw0 = r_vec[1], tx, ty, tz]   (pnp_uncert_cpu.py:68)
    uint8_t *init_mask;     // out (B,P): istd candidates narrowed to the RANSAC inliers (pnp_uncert_cpu.py:43-51)
    uint8_t *init_ok;       // out (B): 0 = the initialiser failed (the reference then returns (False, 0, 0, I, 0, mask), :119-125)
    float *diag;            // out (B,4) or null: RANSAC iterations run, inliers of the best model, candidates, index of the best model
    double *dbg_hyp;        // out (B,30,12) or null: every hypothesis' R (after the Rodrigues round trip) and t — tests
    int max_iters;
    int h0, h1;             // the hypotheses [h0, h1) of this round (round 0: h0 = 0; round 1: the rest, for the objects still pending)
#ifdef MR_DEBUG_STAMPS
    unsigned long long *cstamps;      // development builds: (B,24) cycle stamps of the consensus body (EPC_STAMP), or null
#endif
};

size_t epnp_work_bytes(int B, int P, EpnpWork *w, unsigned char *base) {
    const size_t nq = (size_t)B * kEpMaxIters, ps = (size_t)((P + 7) & ~7);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_meta = take(sizeof(int) * kEpMeta * B), o_samp = take(sizeof(float) * kEpSampRec * nq), o_hrt = take(sizeof(double) * 12 * nq),
                 o_cand = take(sizeof(uint16_t) * ps * B), o_fit = take(sizeof(uint16_t) * ps * B), o_prep_r = take(sizeof(double) * 24 * B),
                 o_mtm_r = take(sizeof(double) * 144 * B), o_cand_r = take(sizeof(double) * kEpCandStride * B), o_cam = take(sizeof(float) * 4 * B), o_abt_r = take(sizeof(double) * 24 * B),
                 o_spt = take(sizeof(uint16_t) * 5 * kEpMaxIters * B), o_bits = take(sizeof(unsigned long long) * ((size_t)(P + 63) >> 6) * B);
    if (w) {
        w->meta = (int *)(base + o_meta); w->samp = (float *)(base + o_samp); w->hrt = (double *)(base + o_hrt); w->cand = (uint16_t *)(base + o_cand);
        w->fit = (uint16_t *)(base + o_fit); w->prep_r = (double *)(base + o_prep_r); w->mtm_r = (double *)(base + o_mtm_r); w->cand_r = (double *)(base + o_cand_r); w->cam = (float *)(base + o_cam); w->abt_r = (double *)(base + o_abt_r);
        w->spt = (uint16_t *)(base + o_spt);
        w->nq = (long long)nq; w->pstride = (int)ps;
        (void)o_bits;                                     // the bit rows follow spt: ep_fitbits()
    }
    return off;
}

// The re-fit's point list once more as a MASK, one bit per point (bit p & 63 of word p >> 6; (P + 63) / 64 words per object, on 8-byte boundaries), for the
// LM launch that carries the re-fit: the last array of the workspace, behind spt (epnp_work_bytes' o_bits).  Located from spt rather than through a
// pointer of its own in EpnpWork: that struct is part of every stage's kernel arguments, and the stages that do not touch the rows keep their code.
__host__ __device__ __forceinline__ unsigned long long *ep_fitbits(const EpnpWork &w, const long long B) {
    return (unsigned long long *)((unsigned char *)w.spt + (((size_t)sizeof(uint16_t) * 5 * kEpMaxIters * (size_t)B + 255) & ~(size_t)255));
}
__host__ __device__ __forceinline__ int ep_fitbits_stride(const int P) { return (P + 63) >> 6; }

// the tensors of the call object b belongs to, as load_records and the camera read them
struct EpCallView {
    const void *x2d, *istd, *x3d, *K;
    const long long *s2, *sw, *s3;
    int vec, K_stride, K_f64;
    const float *ransac_thr;
    double *init_pose; uint8_t *init_mask; uint8_t *init_ok; float *diag;
};
__device__ __forceinline__ EpCallView ep_call_view(const EpnpStageArgs &ea, const int b) {      // b is workgroup-uniform
    EpCallView v;
    v.x2d = ea.p.x2d; v.istd = ea.p.istd; v.x3d = ea.p.x3d; v.K = ea.p.K; v.ransac_thr = ea.p.ransac_thr;
    v.init_pose = ea.init_pose; v.init_mask = ea.init_mask; v.init_ok = ea.init_ok; v.diag = ea.diag;
    if (ea.ncalls > 1) {
        const EpnpCallPtrs &c = ea.call[b / ea.group_B];
        v.x2d = c.x2d; v.istd = c.istd; v.x3d = c.x3d; v.K = c.K; v.ransac_thr = c.ransac_thr;
        v.init_pose = c.init_pose; v.init_mask = c.init_mask; v.init_ok = c.init_ok; v.diag = c.diag;
    }
    v.s2 = ea.p.s2; v.sw = ea.p.sw; v.s3 = ea.p.s3; v.vec = ea.p.vec; v.K_stride = ea.p.K_stride; v.K_f64 = ea.p.K_f64;
    return v;
}
__device__ __forceinline__ EpCam ep_cam_of(const EpCallView &a, int b) {
    double Kall[9];
    ld_k_vec<9>(a.K, a.K_f64, (long long)b * a.K_stride, Kall);
    EpCam cam;
    cam.fx = (double)(float)Kall[0]; cam.fy = (double)(float)Kall[4]; cam.cx = (double)(float)Kall[2]; cam.cy = (double)(float)Kall[5];   // the reference hands cv2 a float32 K
    return cam;
}
// What a stage needs of an object's correspondences, and no more (HBM traffic of one call: 5.4 x the algorithmic bytes with every
// workgroup-per-object launch loading all seven channel rows, profiles/r05a_epnp_traffic.json): the front launch tests the WEIGHTS
// (two rows; A records {0, 0, wu, wv}, no B records) and fetches the first round's sampled correspondences straight from global memory
// (the consensus launch writes a pending object's others from its tile); the consensus launch reads the GEOMETRY into a GeoTile (five
// planar rows), the re-fit launch into Tile's records (A records {u, v, 0, 0}, same layout as load_records).
template <typename T>
__device__ __forceinline__ void ep_load_weights(const EpCallView &a, int b, int P, int NT, const Tile<T> &tl) {
    const T *gw = (const T *)a.istd + (long long)b * a.sw[0];
    Rec4<T> *wa = (Rec4<T> *)const_cast<T *>(tl.ra);
    for (int p = threadIdx.x; p < P; p += NT) {
        Rec4<T> r;
        r.e[0] = r.e[1] = T(0.0f);
        r.e[2] = gw[(long long)p * a.sw[1]]; r.e[3] = gw[(long long)p * a.sw[1] + a.sw[2]];
        wa[p] = r;
    }
}
template <typename T>
__device__ __forceinline__ void ep_load_geometry(const EpCallView &a, int b, int P, int NT, const Tile<T> &tl) {
    const T *g2 = (const T *)a.x2d + (long long)b * a.s2[0];
    const T *g3 = (const T *)a.x3d + (long long)b * a.s3[0];
    Rec4<T> *wa = (Rec4<T> *)const_cast<T *>(tl.ra), *wb = (Rec4<T> *)const_cast<T *>(tl.rb);
    for (int p = threadIdx.x; p < P; p += NT) {
        Rec4<T> ra_, rb_;
        ra_.e[0] = g2[(long long)p * a.s2[1]]; ra_.e[1] = g2[(long long)p * a.s2[1] + a.s2[2]]; ra_.e[2] = ra_.e[3] = T(0.0f);
        rb_.e[0] = g3[(long long)p * a.s3[1]]; rb_.e[1] = g3[(long long)p * a.s3[1] + a.s3[2]]; rb_.e[2] = g3[(long long)p * a.s3[1] + 2 * a.s3[2]]; rb_.e[3] = T(0.0f);
        wa[p] = ra_; wb[p] = rb_;
    }
}
// The consensus launch's geometry tile: five planar rows x, y, z, u, v of np = P rounded up to 8 entries each, in the storage type —
// 20 B per point at fp32 where Tile's two 16-byte records {u, v, 0, 0} {x, y, z, 0} take 32 (15.7 instead of 25.1 KB at P = 784).  A
// wave's reads of a row at consecutive points are 4-byte reads of consecutive words (conflict-free); load() hands out the same raw values.
template <typename T>
struct GeoTile {
    const T *r; int np;
    using Raw = TileRaw<T>;
    __device__ __forceinline__ void load(int p, Raw &o) const {
        o.x = r[p]; o.y = r[np + p]; o.z = r[2 * np + p]; o.u = r[3 * np + p]; o.v = r[4 * np + p];
    }
};
template <typename T>
__device__ __forceinline__ void ep_load_geometry(const EpCallView &a, int b, int P, int NT, const GeoTile<T> &tl) {
    const T *g2 = (const T *)a.x2d + (long long)b * a.s2[0];
    const T *g3 = (const T *)a.x3d + (long long)b * a.s3[0];
    T *w = const_cast<T *>(tl.r);
    const int np = tl.np;
    for (int p = threadIdx.x; p < P; p += NT) {
        const T x = g3[(long long)p * a.s3[1]], y = g3[(long long)p * a.s3[1] + a.s3[2]], z = g3[(long long)p * a.s3[1] + 2 * a.s3[2]];
        const T u = g2[(long long)p * a.s2[1]], v = g2[(long long)p * a.s2[1] + a.s2[2]];
        w[p] = x; w[np + p] = y; w[2 * np + p] = z; w[3 * np + p] = u; w[4 * np + p] = v;
    }
}
// one correspondence straight from global memory, as the float32 values the tile would hand out
template <typename T>
__device__ __forceinline__ void ep_fetch_global(const EpCallView &a, int b, int p, float (&o)[5]) {
    const T *g2 = (const T *)a.x2d + (long long)b * a.s2[0] + (long long)p * a.s2[1];
    const T *g3 = (const T *)a.x3d + (long long)b * a.s3[0] + (long long)p * a.s3[1];
    o[0] = (float)to_f(g3[0]); o[1] = (float)to_f(g3[a.s3[2]]); o[2] = (float)to_f(g3[2 * a.s3[2]]);
    o[3] = (float)to_f(g2[0]); o[4] = (float)to_f(g2[a.s2[2]]);
}

// ... and for the lane-mapped launches, from the workspace (the front launch left the four float32 values there)
__device__ __forceinline__ EpCam ep_cam_ws(const EpnpWork &w, const long long B, const long long b) {
    EpCam cam;
    cam.fx = (double)w.cam[b]; cam.fy = (double)w.cam[B + b]; cam.cx = (double)w.cam[2 * B + b]; cam.cy = (double)w.cam[3 * B + b];
    return cam;
}

// ------------------------------------------------------------------------------------------------ the sample-level pieces of EPnP
// world points and image points as epnp sees them (normalised in float32, back to pixels in double)
__device__ __forceinline__ void ep_points5(const EpCam &k, const float (&obj)[5][3], const float (&img)[5][2], double (&pws)[5][3], double (&us)[5][2]) {
    MR_EXACT
    const double ifx = 1.0 / k.fx, ify = 1.0 / k.fy;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) pws[i][j] = (double)obj[i][j];
        const float xn = (float)(((double)img[i][0] - k.cx) * ifx), yn = (float)(((double)img[i][1] - k.cy) * ify);
        us[i][0] = (double)xn * k.fx + k.cx; us[i][1] = (double)yn * k.fy + k.cy;
    }
}

// control points (centroid + PCA axes) and barycentric coordinates of the five points
// pseudo-inverse of the control-point basis [c1 - c0, c2 - c0, c3 - c0] = the orthonormal PCA axes (rows of uct) scaled by kk_j:
// diag(1 / kk_j) uct, a zero row for a scale that counts as zero (<= 2 eps sum: planar / collinear points) — oracle/epnp.inc epnp_solve
__device__ __forceinline__ void ep_basis_pinv(const double (&kk)[3], const double (&uct)[9], double (&ci)[9]) {
    MR_EXACT
    const double ksum = (kk[0] + kk[1]) + kk[2], thr = 2.0 * 2.220446049250313e-16 * ksum;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double rk = 1.0 / kk[j];
#pragma unroll
        for (int i = 0; i < 3; ++i) ci[3 * j + i] = kk[j] > thr ? uct[3 * j + i] * rk : 0.0;
    }
}

// barycentric coordinates of one world point in the control-point basis (centroid c0, pseudo-inverse ci)
__device__ __forceinline__ void ep_alphas_of(const double (&pw)[3], const double (&c0)[3], const double (&ci)[9], double (&al)[4]) {
    MR_EXACT
#pragma unroll
    for (int j = 0; j < 3; ++j) al[1 + j] = ci[3 * j] * (pw[0] - c0[0]) + ci[3 * j + 1] * (pw[1] - c0[1]) + ci[3 * j + 2] * (pw[2] - c0[2]);
    al[0] = 1.0 - al[1] - al[2] - al[3];
}

__device__ __forceinline__ void ep_prep5(const double (&pws)[5][3], double (&cws)[4][3], double (&alphas)[5][4], double (&ci)[9]) {
    MR_EXACT
#pragma unroll
    for (int j = 0; j < 3; ++j) cws[0][j] = ep_psum5(pws[0][j], pws[1][j], pws[2][j], pws[3][j], pws[4][j]) / 5.0;
    double C[9], dc[3], uct[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double tm[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) tm[i] = fma(pws[i][a] - cws[0][a], pws[i][b] - cws[0][b], 0.0);
            C[3 * a + b] = C[3 * b + a] = ep_psum5(tm[0], tm[1], tm[2], tm[3], tm[4]);
        }
    ep_eig3(C, dc, uct);
    double kv[3];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const double kk = sqrt((dc[i - 1] > 0.0 ? dc[i - 1] : 0.0) / 5.0);
        kv[i - 1] = kk;
#pragma unroll
        for (int j = 0; j < 3; ++j) cws[i][j] = cws[0][j] + kk * uct[3 * (i - 1) + j];
    }
    ep_basis_pinv(kv, uct, ci);
#pragma unroll
    for (int i = 0; i < 5; ++i) ep_alphas_of(pws[i], cws[0], ci, alphas[i]);
}

// ---- scratch the four lanes of a quad share, in LDS: one column per quad of the 64-thread workgroup (16 quads).  Every lane of the quad
// writes the (identical) value it computed and reads back what it needs, so no fence is involved: a lane only ever reads what it wrote
// itself.  What this buys: the 6 x 10 system, rho, the control points and the basis inverse do not occupy registers while the eigen-solver,
// the 6 x 5 SVD and the Gauss-Newton run (round 4 kept them — and the four eigenvectors as 48 doubles per lane — in 478 / 490 registers,
// one wave per SIMD; now lane t keeps eigenvector t and the others' components arrive by quad_perm DPP where they are used).
constexpr int kQL = 0, kQRho = 60, kQCws = 66, kQCi = 78, kQSlots = 87;
constexpr int kEpWideMtm = 0, kEpWideGn = 144, kEpWide = 144 + 4 * 6 * 5;      // doubles of LDS per matrix of a WIDE launch: M^T M rows [12][12], Gauss-Newton rows [lane of the quad][6][5]
struct EpQuadScratch {
    double *p;                                              // this quad's column: slot s lives at p[16 s]
    __device__ __forceinline__ double ld(int slot) const { return p[slot * 16]; }
    __device__ __forceinline__ void st(int slot, double v) const { p[slot * 16] = v; }
};

// the 6 x 10 system of the beta approximations from the quad's four null-space vectors (lane t holds vector t), and rho from the control
// points in the scratch: both into the scratch
// LV > 0 (wide launches; the matrix's quads SHARE one scratch column): row i of L by quad i of the matrix — the four vectors meet in LDS (`wide`: [4][12], where the
// M^T M rows were), the row's pair of control points (a, b) only selects addresses, the ten entries are the quad form's expressions — a sixth of the rows per lane
template <int LV = 0>
__device__ __forceinline__ void ep_L_rho_quad(const double (&z)[12], const EpQuadScratch &sq, double *wide = nullptr, const int sqi = 0) {
    MR_EXACT
    if constexpr (LV > 0) {
        const int jj = threadIdx.x & 3;
#pragma unroll
        for (int c = 0; c < 12; ++c) wide[12 * jj + c] = z[c];            // (every quad of the matrix stores the same values)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        constexpr int NQ = 1 << LV;
#pragma unroll
        for (int tt = 0; tt < (6 + NQ - 1) / NQ; ++tt) {
            const int i = sqi + NQ * tt, ii = i < 6 ? i : 0;
            const int a = ii < 3 ? 0 : (ii < 5 ? 1 : 2), b = ii < 3 ? ii + 1 : (ii < 5 ? ii - 1 : 3);      // the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
            double dv[4][3];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int k = 0; k < 3; ++k) dv[t][k] = wide[12 * t + 3 * a + k] - wide[12 * t + 3 * b + k];
            if (i < 6) {
                sq.st(kQL + 10 * i + 0, ep_dot3(dv[0], dv[0])); sq.st(kQL + 10 * i + 1, 2.0 * ep_dot3(dv[0], dv[1])); sq.st(kQL + 10 * i + 2, ep_dot3(dv[1], dv[1]));
                sq.st(kQL + 10 * i + 3, 2.0 * ep_dot3(dv[0], dv[2])); sq.st(kQL + 10 * i + 4, 2.0 * ep_dot3(dv[1], dv[2])); sq.st(kQL + 10 * i + 5, ep_dot3(dv[2], dv[2]));
                sq.st(kQL + 10 * i + 6, 2.0 * ep_dot3(dv[0], dv[3])); sq.st(kQL + 10 * i + 7, 2.0 * ep_dot3(dv[1], dv[3])); sq.st(kQL + 10 * i + 8, 2.0 * ep_dot3(dv[2], dv[3]));
                sq.st(kQL + 10 * i + 9, ep_dot3(dv[3], dv[3]));
            }
        }
        double c[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[i][k] = sq.ld(kQCws + 3 * i + k);
        sq.st(kQRho + 0, ep_dist2(c[0], c[1])); sq.st(kQRho + 1, ep_dist2(c[0], c[2])); sq.st(kQRho + 2, ep_dist2(c[0], c[3]));
        sq.st(kQRho + 3, ep_dist2(c[1], c[2])); sq.st(kQRho + 4, ep_dist2(c[1], c[3])); sq.st(kQRho + 5, ep_dist2(c[2], c[3]));
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        return;
    }
    int a = 0, b = 1;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double dv[4][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double own = z[3 * a + k] - z[3 * b + k];
#pragma unroll
            for (int t = 0; t < 4; ++t) dv[t][k] = eq4_bcast(own, t);
        }
        sq.st(kQL + 10 * i + 0, ep_dot3(dv[0], dv[0])); sq.st(kQL + 10 * i + 1, 2.0 * ep_dot3(dv[0], dv[1])); sq.st(kQL + 10 * i + 2, ep_dot3(dv[1], dv[1]));
        sq.st(kQL + 10 * i + 3, 2.0 * ep_dot3(dv[0], dv[2])); sq.st(kQL + 10 * i + 4, 2.0 * ep_dot3(dv[1], dv[2])); sq.st(kQL + 10 * i + 5, ep_dot3(dv[2], dv[2]));
        sq.st(kQL + 10 * i + 6, 2.0 * ep_dot3(dv[0], dv[3])); sq.st(kQL + 10 * i + 7, 2.0 * ep_dot3(dv[1], dv[3])); sq.st(kQL + 10 * i + 8, 2.0 * ep_dot3(dv[2], dv[3]));
        sq.st(kQL + 10 * i + 9, ep_dot3(dv[3], dv[3]));
        if (++b > 3) { ++a; b = a + 1; }
    }
    double c[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[i][k] = sq.ld(kQCws + 3 * i + k);
    sq.st(kQRho + 0, ep_dist2(c[0], c[1])); sq.st(kQRho + 1, ep_dist2(c[0], c[2])); sq.st(kQRho + 2, ep_dist2(c[0], c[3]));
    sq.st(kQRho + 3, ep_dist2(c[1], c[2])); sq.st(kQRho + 4, ep_dist2(c[1], c[3])); sq.st(kQRho + 5, ep_dist2(c[2], c[3]));
}

// control points in the camera frame: sum_i beta_i v_i, v_i = the vector lane i of the quad holds
__device__ __forceinline__ void ep_ccs_quad(const double (&z)[12], const double (&betas)[4], double (&ccs)[4][3]) {
    MR_EXACT
#pragma unroll
    for (int j = 0; j < 4; ++j) ccs[j][0] = ccs[j][1] = ccs[j][2] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) ccs[j][k] += betas[i] * eq4_bcast(z[3 * j + k], i);
}

// pose of one beta candidate on the 5 points of a sample: R, t and the mean reprojection error; the barycentric coordinates are
// recomputed from the scratch's control-point basis (the expression ep_prep5 evaluated)
__device__ __forceinline__ void ep_pose5_quad(const EpCam &k, const double (&ccs)[4][3], const EpQuadScratch &sq,
                                              const double (&pws)[5][3], const double (&us)[5][2], double (&R)[9], double (&t)[3], double &rep_err) {
    MR_EXACT
    double pcs[5][3], pw0[3], ci[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) pw0[c] = sq.ld(kQCws + c);
#pragma unroll
    for (int c = 0; c < 9; ++c) ci[c] = sq.ld(kQCi + c);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double al[4];
        ep_alphas_of(pws[i], pw0, ci, al);
#pragma unroll
        for (int j = 0; j < 3; ++j) pcs[i][j] = al[0] * ccs[0][j] + al[1] * ccs[1][j] + al[2] * ccs[2][j] + al[3] * ccs[3][j];
    }
    if (pcs[0][2] < 0.0) {
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) pcs[i][j] = -pcs[i][j];
    }
    double pc0[3], abt[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) pc0[j] = ep_psum5(pcs[0][j], pcs[1][j], pcs[2][j], pcs[3][j], pcs[4][j]) / 5.0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double tm[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) tm[i] = fma(pcs[i][j] - pc0[j], pws[i][c] - pw0[c], 0.0);
            abt[3 * j + c] = ep_psum5(tm[0], tm[1], tm[2], tm[3], tm[4]);
        }
    ep_abt_to_pose(abt, pc0, pw0, R, t);
    double er[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double Xc = ep_dot3(&R[0], pws[i]) + t[0], Yc = ep_dot3(&R[3], pws[i]) + t[1], iz = 1.0 / (ep_dot3(&R[6], pws[i]) + t[2]);
        const double du = us[i][0] - (k.cx + k.fx * Xc * iz), dv = us[i][1] - (k.cy + k.fy * Yc * iz);
        er[i] = sqrt(du * du + dv * dv);
    }
    rep_err = ep_psum5(er[0], er[1], er[2], er[3], er[4]) / 5.0;
}

// beta approximation and Gauss-Newton of this lane's candidate on the system in the scratch (ep_betas_approx_lane / ep_gauss_newton of
// epnp_kernel.inc with L and rho read where they are used)
template <int LV = 0>
__device__ __forceinline__ void ep_betas_quad(const EpQuadScratch &sq, const int cand, double (&be)[4], double *wide = nullptr, const int sqi = 0) {
    MR_EXACT
    {
        double A[30], rho[6], x5[5];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double l2 = sq.ld(kQL + 10 * i + 2), l3 = sq.ld(kQL + 10 * i + 3), l4 = sq.ld(kQL + 10 * i + 4), l6 = sq.ld(kQL + 10 * i + 6);
            A[5 * i] = sq.ld(kQL + 10 * i); A[5 * i + 1] = sq.ld(kQL + 10 * i + 1);
            A[5 * i + 2] = cand == 0 ? l3 : l2;
            A[5 * i + 3] = cand == 0 ? l6 : (cand == 2 ? l3 : 0.0);
            A[5 * i + 4] = cand == 2 ? l4 : 0.0;
            rho[i] = sq.ld(kQRho + i);
        }
        ep_svd_solve<6, 5>(A, rho, x5);
        ep_betas_from_x5(x5, cand, be);
    }
    bool live = true;
    for (int it = 0; it < 5; ++it) {
        if (!live) break;
        asm volatile("" ::: "memory");                      // L and rho are READ here every iteration, not carried in 132 registers across the loop
        double A[24], b[6], x[4];
        if constexpr (LV > 0) {
            // wide launches: the six rows of the system spread over the matrix's quads (row i by quad i mod NQ: the row index only selects addresses), gathered
            // through LDS (`wide + kEpWideGn`: [lane of the quad][row][A0..A3, b]); every lane then holds the same 6 x 4 system the quad form builds
            constexpr int NQ = 1 << LV;
            double *gn = wide + kEpWideGn + (threadIdx.x & 3) * 30;
#pragma unroll
            for (int t = 0; t < (6 + NQ - 1) / NQ; ++t) {
                const int i = sqi + NQ * t;                   // (quads beyond the rows: a valid address, nothing stored)
                const int ii = i < 6 ? i : 0;
                double r[10], ar[4], br;
#pragma unroll
                for (int e = 0; e < 10; ++e) r[e] = sq.p[(kQL + 10 * ii + e) * 16];
                ep_gn_row(r, sq.p[(kQRho + ii) * 16], be, ar, br);
                if (i < 6) { gn[5 * i] = ar[0]; gn[5 * i + 1] = ar[1]; gn[5 * i + 2] = ar[2]; gn[5 * i + 3] = ar[3]; gn[5 * i + 4] = br; }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
            for (int i = 0; i < 6; ++i) { A[4 * i] = gn[5 * i]; A[4 * i + 1] = gn[5 * i + 1]; A[4 * i + 2] = gn[5 * i + 2]; A[4 * i + 3] = gn[5 * i + 3]; b[i] = gn[5 * i + 4]; }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // (read before the next iteration's rows are stored)
        } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double r[10];
#pragma unroll
            for (int e = 0; e < 10; ++e) r[e] = sq.ld(kQL + 10 * i + e);
            ep_gn_row(r, sq.ld(kQRho + i), be, &A[4 * i], b[i]);
            asm volatile("" : "+v"(b[i]));                  // b is formed HERE (the compiler otherwise sinks it behind the QR's success test and keeps 26 partial products alive across the factorisation)
        }
        }
        if (!ep_qr_solve(A, b, x)) live = false;
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i) be[i] += x[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ front
// cv::RNG((uint64)-1), the generator RANSACPointSetRegistrator seeds for every run (ptsetreg.cpp): state = (uint32)state * 4164903690 +
// (state >> 32), next() = (uint32)state.  The seed is fixed, so the stream of 32-bit outputs is a compile-time table; what depends on the
// object is only `% n` and which draws repeat an index of their sample.
constexpr int kEpRngDraws = 512;
struct EpRngTable { unsigned v[kEpRngDraws]; };
constexpr EpRngTable ep_make_rng_table() {
    EpRngTable t{};
    unsigned long long state = ~0ull;
    for (int k = 0; k < kEpRngDraws; ++k) { state = (unsigned long long)(unsigned)state * 4164903690ull + (state >> 32); t.v[k] = (unsigned)state; }
    return t;
}
__constant__ EpRngTable kEpRng = ep_make_rng_table();

size_t epnp_front_lds_bytes(const PnpArgs &a) {
    size_t n = 0;
    n += sizeof(unsigned long long) * a.nca;
    n += sizeof(float) * (4 * a.nla + 4);
    n += (size_t)4 * a.P * a.elem_size;                   // A records only: {0, 0, wu, wv}
    n += sizeof(uint16_t) * ((a.P + 7) & ~7);
    n += sizeof(uint16_t) * 160;
    n += (a.P + 15) & ~15;
    n += sizeof(uint16_t) * kEpRngDraws;
    return (n + 15) & ~(size_t)15;
}

template <typename T>
__global__ void __launch_bounds__(kEpThreads) epnp_front_kernel(const EpnpStageArgs ea) {
    MR_EXACT
    constexpr int WPO = 4, NT = kEpThreads;
    const PnpArgs &a = ea.p;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = a.P;
    const int nchunk = (P + 63) >> 6, npt = (P + NT - 1) / NT;

    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *sball = (unsigned long long *)smem;                  // [nca]
    float *snode = (float *)(sball + a.nca);                                 // [4 * nla]
    float *sres = snode + 4 * a.nla;                                         // [4]
    unsigned char *tile_base = (unsigned char *)(sres + 4);
    Tile<T> tl;
    tl.ra = (const T *)tile_base; tl.rb = nullptr;                           // the weights alone: this launch never looks at a coordinate
    uint16_t *slist = (uint16_t *)(tile_base + (size_t)4 * P * sizeof(T));
    uint16_t *sidx = slist + ((P + 7) & ~7);                                 // [30][5] subset indices (into the candidate list)
    uint8_t *smask = (uint8_t *)(sidx + 160);
    uint16_t *sdraw = (uint16_t *)(smask + ((P + 15) & ~15));               // [512] the generator's outputs modulo n

    const unsigned rng0 = kEpRng.v[tid], rng1 = kEpRng.v[tid + NT];           // this thread's two entries of the generator's stream, in flight behind the tile loads
    const EpCallView cv = ep_call_view(ea, b);
    ep_load_weights<T>(cv, b, P, NT, tl);
    if (tid == 0) {                                       // the camera, for the launches that do not see the caller's tensors
        const EpCam c = ep_cam_of(cv, b);
        ea.w.cam[b] = (float)c.fx; ea.w.cam[(long long)a.B + b] = (float)c.fy; ea.w.cam[2ll * a.B + b] = (float)c.cx; ea.w.cam[3ll * a.B + b] = (float)c.cy;
    }
    int pl_off = 0, pl_len = 0, pl_l = 0, pl_r = 0;
    unsigned pl_ls0 = 0, pl_ls1 = 0;
    if (!(a.flags & MR_NO_ISTD_MASK) && a.mean_mode != MR_MEAN_SEQUENTIAL) {
        if ((lane >> 3) < a.plan.n_leaves) { pl_off = a.plan.leaf_off[lane >> 3]; pl_len = a.plan.leaf_len[lane >> 3]; }
        if (lane < a.plan.n_internal) { pl_l = a.plan.left[lane]; pl_r = a.plan.right[lane]; }
        const unsigned *lsw = (const unsigned *)a.plan.level_start;
        pl_ls0 = lsw[0]; pl_ls1 = lsw[1];
    }
    __syncthreads();
    // ---- istd candidates (pnp_uncert_cpu.py:164-168, :23-32)
    const int n = istd_mask_stage<WPO, T, PnpArgs>(a, tl, P, nchunk, npt, tid, lane, wid, sres, snode, sball, smask, slist, pl_off, pl_len, pl_l, pl_r, pl_ls0, pl_ls1);
    __syncthreads();
    const bool use_ransac = cv.ransac_thr != nullptr;
    // with thresholds, 5 or 4 candidates are solved directly (ptsetreg.cpp: count == modelPoints; four candidates: oracle/epnp.inc decision (ii))
    const int mode = n < 4 ? EP_MODE_FAIL : ((use_ransac && n > 5) ? EP_MODE_RANSAC : EP_MODE_PLAIN);
    if (mode == EP_MODE_RANSAC) {
        // ---- the 30 five-point subsets: cv::RNG((uint64)-1).uniform(0, n) with rejection of repeats (ptsetreg.cpp getSubset).
        // The sequential process (one lane, 150+ dependent multiply / modulo / compare steps: 7.6 us of this launch's 17) as a fixed
        // point: lane `it` of wave 0 takes sample `it` from the draws at its offset into the stream — 5 it to begin with, i.e. no
        // repeats before it — counts the draws it consumed, an exclusive scan of those counts gives every lane its true offset, and the
        // lanes whose offset moved draw again, until nothing moves (lane 0 is right at once, lane k after at most k rounds; a
        // rejection happens in ~2 % of the samples of a 500-candidate set).  Twelve draws per sample at most, 512 per object: beyond
        // either (a handful of candidates: most draws repeat) the sequential loop below runs instead.  Same subsets, bit for bit.
        static_assert(kEpRngDraws == 2 * NT, "two table entries per thread");
        sdraw[tid] = (uint16_t)(rng0 % (unsigned)n); sdraw[tid + NT] = (uint16_t)(rng1 % (unsigned)n);
        __syncthreads();
        bool serial = false;
        if (wid == 0) {
            const bool mine = lane < kEpMaxIters;
            int off = 5 * lane, id0 = -1, id1 = -1, id2 = -1, id3 = -1, id4 = -1;
            bool fail = false;
            for (int round = 0; round <= kEpMaxIters; ++round) {
                int used = 5;
                if (mine && off + 12 <= kEpRngDraws) {
                    int v[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) v[k] = (int)sdraw[off + k];
                    int i = 0;
                    used = 0;
                    id0 = id1 = id2 = id3 = id4 = -1;
#pragma unroll
                    for (int k = 0; k < 12; ++k) {
                        const bool dup = (i > 0 && id0 == v[k]) || (i > 1 && id1 == v[k]) || (i > 2 && id2 == v[k]) || (i > 3 && id3 == v[k]);
                        const bool take = i < 5 && !dup;
                        id0 = (take && i == 0) ? v[k] : id0; id1 = (take && i == 1) ? v[k] : id1; id2 = (take && i == 2) ? v[k] : id2;
                        id3 = (take && i == 3) ? v[k] : id3; id4 = (take && i == 4) ? v[k] : id4;
                        used += i < 5 ? 1 : 0;
                        i += take ? 1 : 0;
                    }
                    fail = i < 5;
                } else fail = mine;
                // exclusive scan of the draws consumed, lanes 0 .. 29
                int incl = mine ? used : 0;
#pragma unroll
                for (int d = 1; d < 32; d <<= 1) { const int t = __shfl_up(incl, d, 64); incl += lane >= d ? t : 0; }
                const int noff = incl - (mine ? used : 0);
                const bool moved = mine && noff != off;
                off = noff;
                if (__ballot(fail) != 0ull) { serial = true; break; }
                if (__ballot(moved) == 0ull) break;
                if (round == kEpMaxIters) serial = true;
            }
            if (!serial && mine) { sidx[lane * 5] = (uint16_t)id0; sidx[lane * 5 + 1] = (uint16_t)id1; sidx[lane * 5 + 2] = (uint16_t)id2; sidx[lane * 5 + 3] = (uint16_t)id3; sidx[lane * 5 + 4] = (uint16_t)id4; }
        }
        if (wid == 0 && serial && lane == 0) {               // the sequential process itself
            unsigned long long state = ~0ull;
            for (int it = 0; it < kEpMaxIters; ++it) {
                int id[5] = { -1, -1, -1, -1, -1 };
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    int v; bool dup;
                    do {
                        state = (unsigned long long)(unsigned)state * 4164903690ull + (state >> 32);
                        v = (int)((unsigned)state % (unsigned)n);
                        dup = false;
#pragma unroll
                        for (int j = 0; j < 5; ++j) dup = dup || (j < i && id[j] == v);
                    } while (dup);
                    id[i] = v;
                    sidx[it * 5 + i] = (uint16_t)v;
                }
            }
        }
        __syncthreads();
        if (tid < 5 * kEpMaxIters) {                     // thread (h, i): correspondence i of sample h -> workspace
            const int h = tid / 5, i = tid - 5 * h;
            const int p = (int)slist[sidx[tid]];
            ea.w.spt[(long long)b * (5 * kEpMaxIters) + tid] = (uint16_t)p;
            if (h < ea.h1) {                             // the first round's samples; a pending object's consensus launch writes the rest
                float o[5];
                ep_fetch_global<T>(cv, b, p, o);
                const long long q = (long long)b * kEpMaxIters + h;
                float *s = ea.w.samp + q * kEpSampRec + 5 * i;
                s[0] = o[0]; s[1] = o[1]; s[2] = o[2]; s[3] = o[3]; s[4] = o[4];
            }
        }
    }
    if (mode != EP_MODE_FAIL) for (int i = tid; i < n; i += NT) ea.w.cand[(long long)b * ea.w.pstride + i] = slist[i];
    for (int p = tid; p < P; p += NT) cv.init_mask[(long long)b * P + p] = smask[p];
    if (tid == 0) {
        int *m = ea.w.meta + (long long)b * kEpMeta;
        m[EP_M_N] = n; m[EP_M_MODE] = mode; m[EP_M_NFIT] = n; m[EP_M_REFIT] = 0; m[EP_M_ITERS] = 0; m[EP_M_BEST] = 0; m[EP_M_BESTH] = -1; m[EP_M_PENDING] = 0; m[EP_M_NITERS] = ea.max_iters > 1 ? ea.max_iters : 1;
    }
}

// quad index of a round -> (object, hypothesis): the round's hypotheses [h0, h1) of every object, compactly; live = the object takes
// part in this round (round 0: every RANSAC object; round 1: the objects whose loop wants more iterations than round 0 had)
__device__ __forceinline__ bool ep_round_lane(const EpnpStageArgs &ea, long long idx, int &b, long long &q) {
    const int nh = ea.h1 - ea.h0;
    const long long total = (long long)ea.p.B * nh;
    if (idx >= total) { b = 0; q = 0; return false; }
    b = (int)(idx / nh);
    q = (long long)b * kEpMaxIters + ea.h0 + (int)(idx - (long long)b * nh);
    const int *m = ea.w.meta + (long long)b * kEpMeta;
    // ... and the hypothesis can still be reached by the object's loop (its iteration bound: the cap in round 0, what round 0 left in round 1)
    return (ea.h0 == 0 ? m[EP_M_MODE] == EP_MODE_RANSAC : m[EP_M_PENDING] != 0) && (int)(q - (long long)b * kEpMaxIters) < m[EP_M_NITERS];
}

constexpr int kEpPoseThreads = 192;     // the re-fit's workgroup: one wave per beta candidate
// ------------------------------------------------------------------------------------------------ hypotheses: sample -> the best candidate's pose
// ONE launch per round, one QUAD per hypothesis (16 hypotheses per single-wave workgroup):
//   control points + barycentric coordinates (the four lanes redundantly: same instruction count as one lane); control points and basis
//   inverse -> the quad's scratch;
//   M^T M: lane j builds rows j, j + 4, j + 8 — the layout the eigen-solver wants, the 12 x 12 never exists anywhere else;
//   the four eigenvectors (epnp_eig_low4.inc; lane t ends up with vector t and keeps it);
//   L, rho -> scratch; lanes 0, 1, 2 = the beta candidates N = 1, 2, 3 (one code path): approximation, Gauss-Newton;
//   pose and reprojection error of each candidate on the sample (re-read from the workspace: 25 floats that nothing kept alive);
//   every candidate lane takes ITS pose through the Rodrigues round trip of solvePnP's output (the consensus launch did this, one thread
//   per hypothesis, with its tile resident in LDS); the candidate with the smallest error (N = 1, 2, 3 in this order, strict <) writes
//   R | t -> workspace: 12 doubles per hypothesis (round 4: 39).
// Registers: 195 (two waves per SIMD, no scratch; 168 = three waves with MR_EP_QUAD_WAVES=3; round 4: 478, one wave per SIMD, which no other
// launch in flight could share).
// cycle stamps of lane 0 of the first 64 workgroups of round 0: development builds only (-DMR_DEBUG_STAMPS, tools/gpu_hyp_timeline.py)
#ifdef MR_DEBUG_STAMPS
#define EP_STAMP(i) do { if (ea.h0 == 0 && ea.p.stamps && threadIdx.x == 0 && blockIdx.x < 64) ea.p.stamps[(long long)blockIdx.x * 24 + (i)] = __builtin_readcyclecounter(); } while (0)
#define EP_EIG_STAMPS (ea.h0 == 0 ? ea.p.stamps : nullptr)
// the consensus body's phases (epnp_consensus_body.inc), thread 0 of EVERY object, into a buffer of its own (the LM launch stamps every object too): 24 per object,
// 12 per round — 0 start | 1 tile loaded | 2 counts done | 3 loop replayed | 4 mask + list done | 5 control points done | 6 moments done | 7 end; 8, 9 = the 100 MHz
// clock at start and end (tools/gpu_consensus_stamps.py)
#define EPC_STAMP(i) do { if (ea.cstamps && threadIdx.x == 0) ea.cstamps[((long long)b * 2 + (ea.h0 > 0 ? 1 : 0)) * 12 + (i)] = (i) >= 8 ? wall_clock64() : __builtin_readcyclecounter(); } while (0)
#else
#define EP_STAMP(i) do { } while (0)
#define EP_EIG_STAMPS nullptr
#define EPC_STAMP(i) do { } while (0)
#endif
#ifndef MR_EP_CONS_WAVES
#define MR_EP_CONS_WAVES 5       // waves per SIMD the consensus launch is compiled for: 5 = 96 registers with 7 spilled (32 B of scratch per lane, all of it in wave 0's control-point
                                 // block: ep_eig3), five objects per CU by registers and 5 x 23.2 KB of LDS (21.9 when this was measured), which leaves 44 KB of the CU to the other streams' workgroups; 4 = 105
                                 // registers, no scratch.  Sets of five on four streams, eight fresh processes each, alternating: 12.30 | 11.91 M solves/s (main: 11.75); in flight
                                 // the LM launch is resident 460 | 514 us (539) — profiles/r07_bench_ab.txt, r07_inflight_trace.txt.  Round 6 (31.8 KB tile): same speed either way
#endif
#ifndef MR_EP_REFIT_WAVES
#define MR_EP_REFIT_WAVES 4
#endif
#ifndef MR_EP_QUAD_WAVES
#define MR_EP_QUAD_WAVES 2       // waves per SIMD the lane-mapped launches are compiled for: 2 = 195 / 204 registers, no scratch; 3 = 168 with ~30 cold spills — within 2 % of each other in flight (profiles/r05_epnp_quad_waves.txt)
#endif

__device__ __forceinline__ void ep_load_sample(const EpnpStageArgs &ea, const long long q, float (&obj)[5][3], float (&img)[5][2]) {
    const float4 *rec = (const float4 *)(ea.w.samp + q * kEpSampRec);
    float v[kEpSampRec];
#pragma unroll
    for (int i = 0; i < kEpSampRec / 4; ++i) { const float4 t = rec[i]; v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w; }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) obj[i][c] = v[5 * i + c];
        img[i][0] = v[5 * i + 3]; img[i][1] = v[5 * i + 4];
    }
}

// one hypothesis q of object b by the quad this lane belongs to; sqcol = the quad's scratch column (slot s at sqcol[16 s]).
// epnp_round2_kernel calls this in a branch only some of its waves take: it must contain no block barrier and no static shared memory.
template <int LV = 0>
__device__ __forceinline__ void ep_hyp_body(const EpnpStageArgs &ea, const int b, const long long q, double *sqcol, const int sqi = 0, double *wide = nullptr) {
    MR_EXACT
    const long long nq = ea.w.nq;
    const int j = threadIdx.x & 3;
    EP_STAMP(0);
    const EpQuadScratch sq{ sqcol };
    const EpCam k = ep_cam_ws(ea.w, ea.p.B, b);
    double z[12];
    {
        float obj[5][3], img[5][2];
        ep_load_sample(ea, q, obj, img);
        double pws[5][3], us[5][2], alphas[5][4], cws[4][3], ci[9];
        ep_points5(k, obj, img, pws, us);
        EP_STAMP(1);
        ep_prep5(pws, cws, alphas, ci);
        EP_STAMP(2);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) sq.st(kQCws + 3 * i + c, cws[i][c]);
#pragma unroll
        for (int c = 0; c < 9; ++c) sq.st(kQCi + c, ci[c]);
        // rows 4 s + j of M^T M: entry (r, c) = psum5 over the points of fma(M2[r], M2[c], fma(M1[r], M1[c], 0)) — the specification's
        // expression for the entry (min(r, c), max(r, c)), products commute.  The non-zero entries of the 5 x 2 rows of M are
        // alpha_ic fx, alpha_ic (cx - u_i), alpha_ic fy, alpha_ic (cy - v_i): alpha and the two image-point products are staged in
        // the scratch (60 doubles, where the reflectors and later L will be) and read where a row or a column needs them — a lane's
        // row index selects an ADDRESS, and no more than one row block and one control point's columns are in registers at a time
        // (round 4 held all of M, 120 doubles, next to the 36 accumulators).
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                sq.st(kQL + 3 * (4 * i + c), alphas[i][c]);
                sq.st(kQL + 3 * (4 * i + c) + 1, alphas[i][c] * (k.cx - us[i][0]));
                sq.st(kQL + 3 * (4 * i + c) + 2, alphas[i][c] * (k.cy - us[i][1]));
            }
        double a[3][12];
        if constexpr (LV > 0) {
            // wide launches: quads 0, 1, 2 of the matrix compute ONE row block each (row 4 q + j: the row index only selects addresses), the rows meet in LDS
            // (`wide`: [12][12]) and every lane reads its three blocks back — a third of the arithmetic per lane; the expressions are the quad form's
            const int sw = sqi < 3 ? sqi : 0;                 // (the matrix's other quads redo block 0 and store nothing)
            double arow[12];
            {
            asm volatile("" ::: "memory");                   // (the staged values are read again for every row block, not kept)
            const int r = 4 * sw + j, cq = (r * 11) >> 5, kk = r - 3 * cq;                // row r = control point cq, coordinate kk
            double m1r[5], m2r[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const double *pq = sq.p + (kQL + 3 * (4 * i + cq)) * 16;
                const double aq = pq[0], zxq = pq[16], zyq = pq[32];
                m1r[i] = kk == 0 ? aq * k.fx : (kk == 1 ? 0.0 : zxq);
                m2r[i] = kk == 0 ? 0.0 : (kk == 1 ? aq * k.fy : zyq);
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                asm volatile("" ::: "memory");
                double ax[5], ay[5], zx[5], zy[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const double al = sq.ld(kQL + 3 * (4 * i + cc));
                    ax[i] = al * k.fx; ay[i] = al * k.fy;
                    zx[i] = sq.ld(kQL + 3 * (4 * i + cc) + 1); zy[i] = sq.ld(kQL + 3 * (4 * i + cc) + 2);
                }
#pragma unroll
                for (int kc = 0; kc < 3; ++kc) {
                    double tm[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const double m1c = kc == 0 ? ax[i] : (kc == 1 ? 0.0 : zx[i]), m2c = kc == 0 ? 0.0 : (kc == 1 ? ay[i] : zy[i]);
                        tm[i] = fma(m2r[i], m2c, fma(m1r[i], m1c, 0.0));
                    }
                    arow[3 * cc + kc] = ep_psum5(tm[0], tm[1], tm[2], tm[3], tm[4]);
                }
                // the three entries are formed HERE (the compiler otherwise sinks the arithmetic below all the loads and spills what they loaded)
                asm volatile("" : "+v"(arow[3 * cc]), "+v"(arow[3 * cc + 1]), "+v"(arow[3 * cc + 2]));
            }
            }
            if (sqi < 3) {
#pragma unroll
                for (int c = 0; c < 12; ++c) wide[(4 * sw + j) * 12 + c] = arow[c];
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int c = 0; c < 12; ++c) a[s][c] = wide[(4 * s + j) * 12 + c];
        } else {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            asm volatile("" ::: "memory");                   // (the staged values are read again for every row block, not kept)
            const int r = 4 * s + j, cq = (r * 11) >> 5, kk = r - 3 * cq;                // row r = control point cq, coordinate kk
            double m1r[5], m2r[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const double *pq = sq.p + (kQL + 3 * (4 * i + cq)) * 16;
                const double aq = pq[0], zxq = pq[16], zyq = pq[32];
                m1r[i] = kk == 0 ? aq * k.fx : (kk == 1 ? 0.0 : zxq);
                m2r[i] = kk == 0 ? 0.0 : (kk == 1 ? aq * k.fy : zyq);
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                asm volatile("" ::: "memory");
                double ax[5], ay[5], zx[5], zy[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const double al = sq.ld(kQL + 3 * (4 * i + cc));
                    ax[i] = al * k.fx; ay[i] = al * k.fy;
                    zx[i] = sq.ld(kQL + 3 * (4 * i + cc) + 1); zy[i] = sq.ld(kQL + 3 * (4 * i + cc) + 2);
                }
#pragma unroll
                for (int kc = 0; kc < 3; ++kc) {
                    double tm[5];
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const double m1c = kc == 0 ? ax[i] : (kc == 1 ? 0.0 : zx[i]), m2c = kc == 0 ? 0.0 : (kc == 1 ? ay[i] : zy[i]);
                        tm[i] = fma(m2r[i], m2c, fma(m1r[i], m1c, 0.0));
                    }
                    a[s][3 * cc + kc] = ep_psum5(tm[0], tm[1], tm[2], tm[3], tm[4]);
                }
                // the three entries are formed HERE (the compiler otherwise sinks the arithmetic below all the loads and spills what they loaded)
                asm volatile("" : "+v"(a[s][3 * cc]), "+v"(a[s][3 * cc + 1]), "+v"(a[s][3 * cc + 2]));
            }
        }
        }
        double lam;
        EP_STAMP(3);
        ep_eig12_low4_quad<LV>(a, z, lam, sq.p + kQL * 16, EP_EIG_STAMPS, sqi);
        EP_STAMP(4);
    }
    const int cand = j == 3 ? 0 : j;
    double be[4];
    ep_L_rho_quad<LV>(z, sq, wide, sqi);
    EP_STAMP(5);
    ep_betas_quad<LV>(sq, cand, be, wide, sqi);
    EP_STAMP(7);
    double R[9], t[3], err;
    {
        double ccs[4][3];
        ep_ccs_quad(z, be, ccs);
        asm volatile("" ::: "memory");                       // the sample is read again, not carried through the solvers
        float obj[5][3], img[5][2];
        ep_load_sample(ea, q, obj, img);
        double pws[5][3], us[5][2];
        ep_points5(k, obj, img, pws, us);
        ep_pose5_quad(k, ccs, sq, pws, us, R, t, err);
    }
    EP_STAMP(8);
    // the Rodrigues round trip of solvePnP's output (rvec out, Rodrigues(rvec) in the RANSAC callback), every candidate lane its own
    double R2[9];
    {
        double rv[3];
        ep_rodrigues_to_vec(R, rv);
        ep_rodrigues_to_mat(rv, R2);
    }
    const double e0 = eq4_bcast(err, 0), e1 = eq4_bcast(err, 1), e2 = eq4_bcast(err, 2);
    int N = 0;
    if (e1 < e0) N = 1;
    if (e2 < (N == 1 ? e1 : e0)) N = 2;
    EP_STAMP(9);
    if (j == N && sqi == 0) {                             // (wide launches: the matrix's other quads computed the same values)
        double *o = ea.w.hrt + q;
#pragma unroll
        for (int i = 0; i < 9; ++i) o[i * nq] = R2[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o[(9 + i) * nq] = t[i];
        if (ea.dbg_hyp) {
#pragma unroll
            for (int i = 0; i < 12; ++i) ea.dbg_hyp[q * 12 + i] = i < 9 ? R2[i] : t[i - 9];
        }
    }
}

// LV = 0: a quad per hypothesis, 16 per wave (launch sets in flight, large calls: instruction count is what they pay for); LV = 2 / 4 ("wide": 4 / 16 quads per
// hypothesis, i.e. a 16-lane row / a whole wave): launches that would leave most of the chip's 1024 SIMDs without a wave — the hypothesis' latency chain is
// what such a launch lasts, and the extra quads shorten it (ep_eig12_low4_quad: LV levels of the bisection per round).  Same values, bit for bit.
// (Also tried on the extra quads, bit-identical and no faster: the two column-disjoint pairs of a Jacobi round of the 6 x 5 systems on two quads, columns in
//  LDS between the rounds — a round is bounded by the rotation's two square roots and division, not by its dot products: profiles/r06_wide_sweep.txt.)
template <int LV>
__global__ void __launch_bounds__(64, MR_EP_QUAD_WAVES) epnp_hyp_kernel(const EpnpStageArgs ea) {
    int b; long long q;
    const long long gq = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    if (!ep_round_lane(ea, gq >> LV, b, q)) return;     // whole hypotheses leave
    __shared__ double sqmem[kQSlots][16];
    __shared__ double widemem[LV > 0 ? kEpWide * (16 >> LV) : 1];      // wide: per matrix of the wave, what its quads exchange (M^T M rows, Gauss-Newton rows)
    double *wide = nullptr;
    if constexpr (LV > 0) wide = widemem + (size_t)((threadIdx.x >> 2) >> LV) * kEpWide;
    ep_hyp_body<LV>(ea, b, q, &sqmem[0][((threadIdx.x >> 2) >> LV) << LV], (int)(gq & ((1 << LV) - 1)), wide);      // (wide: the matrix's quads share its first quad's column — they store the same values)
}

// ------------------------------------------------------------------------------------------------ consensus + the re-fit's sums
constexpr int kEpKeptBallots = 10;      // rounds of at most this many hypotheses keep the counting loop's ballots (launch sets: 3, one call at a time: 10)
__host__ __device__ inline size_t epnp_consensus_tile_bytes(const PnpArgs &a) {      // from the tile's base: GeoTile, the two lists, the inlier mask
    const size_t np = (size_t)((a.P + 7) & ~7);
    return 5 * np * a.elem_size + 2 * sizeof(uint16_t) * np + sizeof(unsigned) * ((a.P + 31) >> 5);
}
size_t epnp_consensus_lds_bytes(const PnpArgs &a) {      // 23.2 KB at P = 784, fp32 (rounds 7 to 9: 21.9, round 6: 31.8)
    size_t n = 0;
    n += sizeof(double) * (30 * 12);
    n += sizeof(unsigned long long) * a.nca;
    n += sizeof(int) * (4 * 32 + 4);
    n += (epnp_consensus_tile_bytes(a) + 7) & ~(size_t)7; // GeoTile, 2 lists of uint16, inlier mask (one bit per point); the ballots below on an 8-byte boundary
    n += sizeof(unsigned long long) * kEpKeptBallots * a.nca;      // the kept ballots: 1.25 KB at P = 784
    return (n + 15) & ~(size_t)15;
}

// one correspondence of the re-fit's set: world point, barycentric coordinates, image point as epnp sees it
template <typename T, typename TL = Tile<T>>
struct EpRefitPoint {
    const TL &tl; const uint16_t *list; const EpCam &cam; const double (&cws)[4][3]; const double (&ci)[9]; double ifx, ify;
    bool norm_f64;          // solvePnPRansac's re-fit: the inliers were converted to CV_64F, the normalised image points stay float64 (oracle/epnp.inc, decision (i))
    __device__ __forceinline__ void operator()(int i, double (&pw)[3], double (&al)[4], double (&uu)[2]) const {
        MR_EXACT
        typename TL::Raw r;
        tl.load((int)list[i], r);
        const float o[3] = { (float)to_f(r.x), (float)to_f(r.y), (float)to_f(r.z) }, im[2] = { (float)to_f(r.u), (float)to_f(r.v) };
#pragma unroll
        for (int j = 0; j < 3; ++j) pw[j] = (double)o[j];
        const double xd = ((double)im[0] - cam.cx) * ifx, yd = ((double)im[1] - cam.cy) * ify;
        const double xn = norm_f64 ? xd : (double)(float)xd, yn = norm_f64 ? yd : (double)(float)yd;
        uu[0] = xn * cam.fx + cam.cx; uu[1] = yn * cam.fy + cam.cy;
#pragma unroll
        for (int j = 0; j < 3; ++j) al[1 + j] = ci[3 * j] * (pw[0] - cws[0][0]) + ci[3 * j + 1] * (pw[1] - cws[0][1]) + ci[3 * j + 2] * (pw[2] - cws[0][2]);
        al[0] = 1.0 - al[1] - al[2] - al[3];
    }
    __device__ __forceinline__ void world(int i, double (&pw)[3]) const {        // the world point alone
        typename TL::Raw r;
        tl.load((int)list[i], r);
        pw[0] = (double)(float)to_f(r.x); pw[1] = (double)(float)to_f(r.y); pw[2] = (double)(float)to_f(r.z);
    }
};

// The re-fit's M^T M (12 x 12, M = the 2n x 12 system of the n inliers) from MOMENT SUMS.  Row 2i of M is [a_k fx, 0, a_k du_i]_k, row
// 2i+1 is [0, a_k fy, a_k dv_i]_k (a = barycentric coordinates, du = cx - u, dv = cy - v), so the 3 x 3 block (c, d) of M^T M is
//     [ fx^2 S0   0        fx Su ]      S0 = sum a_c a_d        Su = sum a_c a_d du
//     [ 0         fy^2 S0  fy Sv ]      Sv = sum a_c a_d dv     Sr = sum a_c a_d (du^2 + dv^2)
//     [ fx Su     fy Sv    Sr    ]
// — 40 sums for the ten pairs c <= d instead of 78 entries (and their ~20 structural-zero products) per point; the restatement
// (oracle/epnp.inc epnp_solve, `moments`) computes the re-fit's M^T M the same way, operation for operation.  Wave W owns the pairs
// p = W mod 4 (p enumerates c <= d row by row): 64 interleaved partials per sum, the butterfly combines them.
// The same pass collects what the re-fit's ABSOLUTE ORIENTATION needs of the points (ep_refit_object): the camera-frame point of a candidate is
// pc = sum_j a_j ccs_j, LINEAR in the barycentric coordinates, so the centroid and the 3 x 3 correlation of every candidate follow from
// sum a_j (4), sum a_j (pw - pw0) (4 x 3) and sum (pw - pw0) (3) — wave W: control point W's four sums and component W of the last —
// instead of two passes over the inliers per candidate; ext = { sum a_W, sum a_W q_0, sum a_W q_1, sum a_W q_2, sum q_W (W < 3) },
// afirst = the first inlier's coordinates (lane 0 of wave 0: the sign test of the candidates' first camera-frame point).
template <int W, typename T, typename TL>
__device__ __forceinline__ void ep_mtm_part(const EpRefitPoint<T, TL> &point, const EpCam &camu, const double (&pw0)[3], const int nn, const int lane,
                                            double (&acc)[12], double (&ext)[5], double (&afirst)[4]) {
    MR_EXACT
    constexpr int NP = W < 2 ? 3 : 2;                     // pairs W, W + 4 (, W + 8)
    constexpr int PC[10] = { 0, 0, 0, 0, 1, 1, 1, 2, 2, 3 }, PD[10] = { 0, 1, 2, 3, 1, 2, 3, 2, 3, 3 };
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) ext[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) afirst[i] = 0.0;
    for (int i = lane; i < nn; i += 64) {
        double pw[3], al[4], uu[2];
        point(i, pw, al, uu);
        const double du = camu.cx - uu[0], dv = camu.cy - uu[1];
        const double rr = fma(du, du, dv * dv);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const double q = al[PC[W + 4 * j]] * al[PD[W + 4 * j]];
            acc[4 * j] += q;
            acc[4 * j + 1] = fma(q, du, acc[4 * j + 1]);
            acc[4 * j + 2] = fma(q, dv, acc[4 * j + 2]);
            acc[4 * j + 3] = fma(q, rr, acc[4 * j + 3]);
        }
        const double q3[3] = { pw[0] - pw0[0], pw[1] - pw0[1], pw[2] - pw0[2] };
        ext[0] += al[W];
#pragma unroll
        for (int k = 0; k < 3; ++k) ext[1 + k] = fma(al[W], q3[k], ext[1 + k]);
        if constexpr (W < 3) ext[4] += q3[W];
        if (W == 0 && i == 0) { afirst[0] = al[0]; afirst[1] = al[1]; afirst[2] = al[2]; afirst[3] = al[3]; }
    }
    wave_allreduce<12>(acc);
    wave_allreduce<5>(ext);
}
template <int W>
__device__ __forceinline__ void ep_abt_store(const double (&ext)[5], const double (&afirst)[4], double *abt_r, const long long B, const int b) {
    abt_r[(long long)b * 24 + W] = ext[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) abt_r[(long long)b * 24 + (4 + 3 * W + k)] = ext[1 + k];
    if constexpr (W < 3) abt_r[(long long)b * 24 + (16 + W)] = ext[4];
    if constexpr (W == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) abt_r[(long long)b * 24 + (20 + j)] = afirst[j];
    }
}
template <int W>
__device__ __forceinline__ void ep_mtm_store(const double (&acc)[12], const EpCam &camu, double *mtm_r, const long long B, const int b) {
    MR_EXACT
    constexpr int NP = W < 2 ? 3 : 2;
    constexpr int PC[10] = { 0, 0, 0, 0, 1, 1, 1, 2, 2, 3 }, PD[10] = { 0, 1, 2, 3, 1, 2, 3, 2, 3, 3 };
    const double fx2 = camu.fx * camu.fx, fy2 = camu.fy * camu.fy;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int c = PC[W + 4 * j], d = PD[W + 4 * j];
        const double blk[3][3] = { { fx2 * acc[4 * j], 0.0, camu.fx * acc[4 * j + 1] },
                                   { 0.0, fy2 * acc[4 * j], camu.fy * acc[4 * j + 2] },
                                   { camu.fx * acc[4 * j + 1], camu.fy * acc[4 * j + 2], acc[4 * j + 3] } };
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mtm_r[(long long)b * 144 + (12 * (3 * c + i) + 3 * d + k)] = blk[i][k];
                if (c != d) mtm_r[(long long)b * 144 + (12 * (3 * d + k) + 3 * c + i)] = blk[i][k];
            }
    }
}

// WPO = waves per object: 4, the one instantiation (two measured slower in every regime: profiles/r05_epnp_grouping.txt)
template <typename T, int WPO>
__global__ void __launch_bounds__(64 * WPO, MR_EP_CONS_WAVES) epnp_consensus_kernel(const EpnpStageArgs ea) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int b = blockIdx.x;
    {
#include "epnp_consensus_body.inc"
    }
}

// ------------------------------------------------------------------------------------------------ the second round as ONE launch (small launch sets)
// One call at a time the second round idles in 97 % of config-2 batches (first round of 10), and an idle launch still costs its ~5 us: two of them
// per call (profiles/r06_epnp_launches.txt).  For launch sets of fewer than 2048 objects the round is one launch: a workgroup per object that
// leaves at once unless the object's replayed loop wants more; otherwise the quads of its first two waves solve the remaining hypotheses
// [h0, h1) (at most 32: h0 >= 1 ... the library's first round is >= 3), the results go through the workspace as in the two-launch form, and the
// whole workgroup runs the consensus body on them.  Same functions, same values; a pending object holds the consensus tile's LDS through its
// hypotheses' latency chain, which is why launch sets in flight keep the two compact launches (residency x time is what they compete for).
constexpr int kEpRound2Quads = 32;
size_t epnp_round2_lds_bytes(const PnpArgs &a) {
    const size_t c = epnp_consensus_lds_bytes(a), h = sizeof(double) * kQSlots * 16 * (kEpRound2Quads / 16);
    return c > h ? c : h;
}
template <typename T>
__global__ void __launch_bounds__(256, MR_EP_QUAD_WAVES) epnp_round2_kernel(const EpnpStageArgs ea) {
    constexpr int WPO = 4;
    extern __shared__ __align__(16) unsigned char smem[];
    const int b = blockIdx.x;
    {
        const int *m = ea.w.meta + (long long)b * kEpMeta;
        if (m[EP_M_MODE] != EP_MODE_RANSAC || m[EP_M_PENDING] == 0) return;       // workgroup-uniform
        const int quad = threadIdx.x >> 2, h = ea.h0 + quad;
        if (quad < kEpRound2Quads && h < ea.h1 && h < m[EP_M_NITERS])           // (hypotheses at or beyond the loop's bound: nothing can reach them, ep_round_lane)
            ep_hyp_body(ea, b, (long long)b * kEpMaxIters + h, (double *)smem + (size_t)(threadIdx.x >> 6) * kQSlots * 16 + ((threadIdx.x & 63) >> 2));
        __threadfence();                                                          // the hypotheses' R | t are re-read from the workspace by other lanes of this workgroup
        __syncthreads();
    }
    {
#include "epnp_consensus_body.inc"
    }
}

// ------------------------------------------------------------------------------------------------ the re-fit's eigenvectors and beta candidates
// one QUAD per object: the four eigenvectors of the re-fit's M^T M (lane t: vector t), then lanes 0, 1, 2 = the candidates N = 1, 2, 3
// (one code path): beta approximation, Gauss-Newton, the candidates' control points in the camera frame, their absolute orientation and
// yaw -> workspace (cand_r).  The pose needs only the consensus launch's moments, none of the tile: computed here, four lanes of a quad per
// object, instead of in the prologue of the workgroup-per-object launch that evaluates the candidates (round 8).
// With pc = sum_j a_j ccs_j the camera-frame centroid is pc0 = (sum_j S_j ccs_j) / n and the correlation sum (pc - pc0)(pw - pw0)^T is
// sum_j ccs_j A_j^T - pc0 E^T (S_j = sum a_j, A_j = sum a_j (pw - pw0), E = sum (pw - pw0): ep_mtm_part); the first inlier must lie in
// front of the camera, else the candidate's control points change sign.
template <int LV>
__global__ void __launch_bounds__(64, MR_EP_QUAD_WAVES) epnp_refit_betas_kernel(const EpnpStageArgs ea) {
    MR_EXACT
    const long long B = ea.p.B;
    const int j = threadIdx.x & 3;
    const long long gq = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    const long long b = gq >> LV;                                            // LV > 0: 2^LV quads per object (see epnp_hyp_kernel)
    const int sqi = (int)(gq & ((1 << LV) - 1));
    if (b >= B || ea.w.meta[b * kEpMeta + EP_M_REFIT] == 0) return;          // whole objects leave
    __shared__ double sqmem[kQSlots][16];
    const EpQuadScratch sq{ &sqmem[0][((threadIdx.x >> 2) >> LV) << LV] };                  // (wide: one column per matrix, shared by its quads)
#pragma unroll
    for (int i = 0; i < 12; ++i) sq.st(kQCws + i, ea.w.prep_r[(long long)b * 24 + i]);
    double z[12];
    {
        double a[3][12], lam;
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int c = 0; c < 12; ++c) a[s][c] = ea.w.mtm_r[(long long)b * 144 + (12 * (4 * s + j) + c)];
        ep_eig12_low4_quad<LV>(a, z, lam, sq.p + kQL * 16, nullptr, sqi);
    }
    const int cand = j == 3 ? 0 : j;
    double be[4];
    __shared__ double widemem[LV > 0 ? kEpWide * (16 >> LV) : 1];
    double *wide = nullptr;
    if constexpr (LV > 0) wide = widemem + (size_t)((threadIdx.x >> 2) >> LV) * kEpWide;
    ep_L_rho_quad<LV>(z, sq, wide, sqi);
    ep_betas_quad<LV>(sq, cand, be, wide, sqi);
    double ccs[4][3];
    ep_ccs_quad(z, be, ccs);
    double R[9], t[3], rv[3];
    {
        const double *ab = ea.w.abt_r + b * 24;
        double S[4], A[4][3], E[3], af[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { S[k] = ab[k]; af[k] = ab[20 + k]; }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) A[k][c] = ab[4 + 3 * k + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) E[c] = ab[16 + c];
        const double dn = (double)ea.w.meta[b * kEpMeta + EP_M_NFIT];          // = the inliers the LM launch lists from init_mask
        const double zf = af[0] * ccs[0][2] + af[1] * ccs[1][2] + af[2] * ccs[2][2] + af[3] * ccs[3][2];
        if (zf < 0.0) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) ccs[k][c] = -ccs[k][c];
        }
        double pc0[3], abt[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) pc0[r] = (S[0] * ccs[0][r] + S[1] * ccs[1][r] + S[2] * ccs[2][r] + S[3] * ccs[3][r]) / dn;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                abt[3 * r + c] = fma(-pc0[r], E[c], fma(ccs[3][r], A[3][c], fma(ccs[2][r], A[2][c], fma(ccs[1][r], A[1][c], ccs[0][r] * A[0][c]))));
        const double pw0[3] = { ea.w.prep_r[b * 24], ea.w.prep_r[b * 24 + 1], ea.w.prep_r[b * 24 + 2] };
        ep_abt_to_pose(abt, pc0, pw0, R, t);
        ep_rodrigues_to_vec(R, rv);
    }
    if (j < 3 && sqi == 0) {
        double *rec = ea.w.cand_r + b * kEpCandStride + kEpCandRec * cand;
#pragma unroll
        for (int i = 0; i < 9; ++i) rec[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) rec[9 + i] = t[i];
        rec[12] = rv[1];
    }
}

// ------------------------------------------------------------------------------------------------ the re-fit's candidates, outputs
constexpr int kEpRefitScratch = 16;                 // doubles of LDS ep_refit_object works in: error | yaw | t of the three candidates (15, padded)
size_t epnp_refit_lds_bytes(const PnpArgs &a) {
    size_t n = 0;
    n += sizeof(double) * kEpRefitScratch;
    n += (size_t)8 * a.P * a.elem_size;
    n += sizeof(uint16_t) * ((a.P + 7) & ~7);
    return (n + 15) & ~(size_t)15;
}

// what the initialiser hands to its caller for object b: start pose, success flag, diagnostics (one thread)
__device__ __forceinline__ void ep_store_init(uint8_t *init_ok, double *init_pose, float *diag, const int b, const bool ok, const double (&pose)[4], const int *meta) {
    init_ok[b] = ok ? 1 : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) init_pose[(long long)b * 4 + j] = ok ? pose[j] : 0.0;
    if (diag) {
        const bool ransac = meta[EP_M_MODE] == EP_MODE_RANSAC;
        diag[(long long)b * 4 + 0] = (float)meta[EP_M_ITERS]; diag[(long long)b * 4 + 1] = (float)(ransac ? meta[EP_M_BEST] : meta[EP_M_NFIT]);
        diag[(long long)b * 4 + 2] = (float)meta[EP_M_N]; diag[(long long)b * 4 + 3] = (float)meta[EP_M_BESTH];
    }
}

// The mean reprojection error over the inliers of the NC candidates c0, c0 + step, ... (< 3) of one wave, in ONE pass over the inliers:
// each point is fetched once and feeds NC accumulators, each of them the per-lane sum the one-candidate pass forms (same terms, same
// order), reduced by a wave_allreduce<1> of its own — the candidate's sum is one wave's 64 interleaved partials + butterfly whatever NC is.
// Lane 0 leaves error, yaw and t of each candidate in scand[5 c ..].
template <int NC, typename T, typename TL>
__device__ __forceinline__ void ep_refit_errors(const EpRefitPoint<T, TL> &point, const EpCam &camu, const double *rec, const int c0, const int step,
                                                const int nn, const double dn, const int lane, double *scand, unsigned long long *dbg_st = nullptr) {
    MR_EXACT
    double R[NC][9], t[NC][3], s[NC][1];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const double *r = rec + kEpCandRec * (c0 + k * step);
#pragma unroll
        for (int i = 0; i < 9; ++i) R[k][i] = r[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[k][i] = r[9 + i];
        s[k][0] = 0.0;
    }
#ifdef MR_DEBUG_STAMPS          // development builds (tools/gpu_lm_handover_stamps.py): the prologue's inputs — prep_r, the candidates' records — have arrived
    if (dbg_st) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); if (threadIdx.x == 0) dbg_st[10] = __builtin_readcyclecounter(); }
#endif
    for (int i = lane; i < nn; i += 64) {
        double pw[3], al[4], uu[2];
        point(i, pw, al, uu);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const double Xc = ep_dot3(&R[k][0], pw) + t[k][0], Yc = ep_dot3(&R[k][3], pw) + t[k][1], iz = 1.0 / (ep_dot3(&R[k][6], pw) + t[k][2]);
            const double du = uu[0] - (camu.cx + camu.fx * Xc * iz), dv = uu[1] - (camu.cy + camu.fy * Yc * iz);
            s[k][0] += sqrt(du * du + dv * dv);
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        wave_allreduce<1>(s[k]);
        const int c = c0 + k * step;
        if (lane == 0) {
            scand[5 * c] = s[k][0] / dn; scand[5 * c + 1] = rec[kEpCandRec * c + 12];
            scand[5 * c + 2] = t[k][0]; scand[5 * c + 3] = t[k][1]; scand[5 * c + 4] = t[k][2];
        }
    }
}

// The re-fit of ONE object by the waves of its workgroup (every wave of the workgroup calls this: one barrier inside): reprojection error
// over the inliers `slist[0..nn)` of the tile `tl` of the three beta candidates whose poses refit_betas left in the workspace (cand_r);
// the best candidate's pose (yaw, t) to every thread.  Shared by epnp_refit_kernel (three waves, geometry tile) and by the LM launch that
// carries the re-fit as its prologue (pnp_uncert_refit_kernel: WPO waves, the LM's own tile) — candidate c is wave c mod NW's (a wave that
// owns two or three evaluates them in one pass, ep_refit_errors), every sum is one wave's 64 interleaved partials + butterfly whichever wave
// that is, so both give the same bits.  (Up to round 7 the candidates' absolute orientation and the best one's Rodrigues vector ran here, on
// three lanes of wave 0 while the other waves waited at a barrier.)
//   scand: [3][5] doubles of LDS (error, yaw, t of the candidates).
//   prep: the object's 24 doubles of prep_r (centroid, inverse basis), rec: its candidate records (cand_r) — in the workspace (epnp_refit_kernel) or where the
//   caller parked them in LDS (the LM launch loads them with its tile); the same values, the same arithmetic.
template <typename T, int NW, typename TL>
__device__ __forceinline__ bool ep_refit_object(const TL &tl, const uint16_t *slist, const int nn, double *scand, const EpCam &cam, const double *prep,
                                                const double *rec, const bool norm_f64, const int wid, const int lane, double (&pose)[4],
                                                unsigned long long *dbg_st = nullptr) {
    MR_EXACT
    double cws[4][3], ci[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) { cws[0][j] = uni(prep[j]); cws[1][j] = cws[2][j] = cws[3][j] = 0.0; }     // only the centroid is needed here
#pragma unroll
    for (int i = 0; i < 9; ++i) ci[i] = uni(prep[12 + i]);
    const double dn = (double)nn;
    EpCam camu;
    camu.fx = uni(cam.fx); camu.fy = uni(cam.fy); camu.cx = uni(cam.cx); camu.cy = uni(cam.cy);
    const EpRefitPoint<T, TL> point{ tl, slist, camu, cws, ci, uni(1.0 / cam.fx), uni(1.0 / cam.fy), norm_f64 };
    if constexpr (NW >= 3) {                              // one candidate per wave (waves 3.. idle)
        if (wid < 3) ep_refit_errors<1, T>(point, camu, rec, wid, NW, nn, dn, lane, scand, dbg_st);
    } else if constexpr (NW == 2) {                       // wave 0: candidates 0 and 2, wave 1: candidate 1
        if (wid == 0) ep_refit_errors<2, T>(point, camu, rec, 0, 2, nn, dn, lane, scand, dbg_st);
        else ep_refit_errors<1, T>(point, camu, rec, 1, 2, nn, dn, lane, scand);
    } else {
        ep_refit_errors<3, T>(point, camu, rec, 0, 1, nn, dn, lane, scand, dbg_st);
    }
    __syncthreads();
    int N = 0;
    if (scand[5] < scand[0]) N = 1;
    if (scand[10] < scand[N * 5]) N = 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) pose[j] = scand[N * 5 + 1 + j];
    return isfinite(pose[0]) && isfinite(pose[1]) && isfinite(pose[2]) && isfinite(pose[3]);
}

template <typename T>
__global__ void __launch_bounds__(kEpPoseThreads, MR_EP_REFIT_WAVES) epnp_refit_kernel(const EpnpStageArgs ea) {
    MR_EXACT
    constexpr int NT = kEpPoseThreads;
    const PnpArgs &a = ea.p;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = a.P;
    const int *meta = ea.w.meta + (long long)b * kEpMeta;
    const int n = meta[EP_M_N], mode = meta[EP_M_MODE], nn = meta[EP_M_NFIT];
    bool ok = meta[EP_M_REFIT] != 0;
    const EpCallView cv = ep_call_view(ea, b);
    double pose[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (ok) {                                             // block-uniform
        extern __shared__ __align__(16) unsigned char smem[];
        double *scand = (double *)smem;                                          // [3][5]
        unsigned char *tile_base = (unsigned char *)(scand + kEpRefitScratch);
        Tile<T> tl;
        tl.ra = (const T *)tile_base; tl.rb = (const T *)tile_base + (size_t)4 * P;
        uint16_t *slist = (uint16_t *)(tile_base + (size_t)8 * P * sizeof(T));
        ep_load_geometry<T>(cv, b, P, NT, tl);
        for (int i = tid; i < nn; i += NT) slist[i] = ea.w.fit[(long long)b * ea.w.pstride + i];
        const EpCam cam = ep_cam_of(cv, b);
        __syncthreads();
        ok = ep_refit_object<T, NT / 64>(tl, slist, nn, scand, cam, ea.w.prep_r + (long long)b * 24, ea.w.cand_r + (long long)b * kEpCandStride, (meta[EP_M_REFIT] & 2) != 0, wid, lane, pose);
    }
    if (tid == 0) ep_store_init(cv.init_ok, cv.init_pose, cv.diag, b, ok, pose, meta);
}

// ------------------------------------------------------------------------------------------------ the LM launch that carries the re-fit
// mr_pnp_uncert_from_epnp_grouped: the initialiser ran with MR_EPNP_DEFER_REFIT (no epnp_refit_kernel launch); this launch loads the
// object's tile ONCE for the re-fit's pose candidates and the LM (one launch, one tile read and one workgroup residency less per call).
// The body is pnp_uncert_kernel's (EXT) with ep_refit_object where that reads init_pose; init_pose / init_valid / the initialiser's
// diagnostics are still written, for the caller.
struct EpnpRefitIn {
    EpnpWork w;                     // the initialiser's workspace
    long long B;                    // objects of the launch set: stride of the workspace's per-object rows
    float *diag[kEpMaxGroup];       // per call (biased like the call table's pointers), or null
};
template <typename T, int WPO>
__global__ void __launch_bounds__(64 * WPO, (std::is_same<T, double>::value ? MR_MIN_WAVES : (WPO <= MR_RELAXED_WPO ? 3 : MR_MIN_WAVES_F32))) pnp_uncert_refit_kernel(const PnpArgs aa, const PnpCallTable tbl, const EpnpRefitIn rf) {
    constexpr bool EXT = true;
    constexpr int NT = 64 * WPO;
    const int b = blockIdx.x;
    const int call_of_b = b / tbl.group_B;
    PnpArgs a = aa;
    {
        const PnpCallTable::CallPtrs &c = tbl.call[call_of_b];
        a.x2d = c.x2d; a.istd = c.istd; a.x3d = c.x3d; a.K = c.K; a.ur = c.ur; a.vr = c.vr;
        a.init_pose = c.init_pose; a.init_mask = c.init_mask; a.init_valid = c.init_valid;
        a.valid = c.valid; a.pose = c.pose; a.cov = c.cov; a.tr = c.tr; a.mask = c.mask; a.diag = c.diag; a.cov_calib = c.cov_calib;
    }
#define MR_K1_KARGS aa
#define MR_K1_REFIT rf
#include "pnp_kernel_body.inc"
#undef MR_K1_REFIT
#undef MR_K1_KARGS
}
