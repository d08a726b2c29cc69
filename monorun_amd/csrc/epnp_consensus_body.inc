// epnp_consensus_body.inc — the body of the consensus stage (csrc/epnp_stages.inc), included TEXTUALLY by the kernels that run it
// (epnp_consensus_kernel<T, WPO>, epnp_round2_kernel<T>): as a function taking the dynamic LDS as a pointer argument the same text compiled to
// 26 spilled registers and 1.7 KB of scratch per lane (the address space of the tile was no longer known), as kernel text it is what round 5
// tuned.  Expects in scope: T, WPO, `ea` (EpnpStageArgs), `b` (the object), `smem` (the kernel's extern __shared__ array).  `return` leaves the kernel.
    MR_EXACT
    constexpr int NT = 64 * WPO;
    const PnpArgs &a = ea.p;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = a.P;
    int *meta = ea.w.meta + (long long)b * kEpMeta;
    const int n = meta[EP_M_N], mode = meta[EP_M_MODE];
    if (mode == EP_MODE_FAIL) return;
    if (ea.h0 > 0 && meta[EP_M_PENDING] == 0) return;                       // second round: only the objects whose loop wants more

    double *shyp = (double *)smem;                                           // [12][30]
    unsigned long long *sball = (unsigned long long *)(shyp + 30 * 12);      // [nca]
    int *scnt = (int *)(sball + a.nca);                                      // [4][32] (+4)
    unsigned char *tile_base = (unsigned char *)(scnt + 4 * 32 + 4);
    const int np = (P + 7) & ~7;
    GeoTile<T> tl;
    tl.r = (const T *)tile_base; tl.np = np;
    uint16_t *slist = (uint16_t *)(tile_base + (size_t)5 * np * sizeof(T));
    uint16_t *slist2 = slist + np;
    unsigned *smask = (unsigned *)(slist2 + np);                            // [(P + 31) / 32]: the inlier mask, one bit per point
    // [kEpKeptBallots][nca]: the counting loop's ballots, per hypothesis of the round and 64-candidate chunk (rounds of at most kEpKeptBallots hypotheses)
    unsigned long long *sbal_h = (unsigned long long *)(tile_base + ((epnp_consensus_tile_bytes(a) + 7) & ~(size_t)7));

    EPC_STAMP(8); EPC_STAMP(0);
    const EpCallView cv = ep_call_view(ea, b);
    ep_load_geometry<T>(cv, b, P, NT, tl);
    for (int i = tid; i < n; i += NT) slist[i] = ea.w.cand[(long long)b * ea.w.pstride + i];
    const EpCam cam = ep_cam_of(cv, b);
    const float thr_given = cv.ransac_thr ? cv.ransac_thr[b] : 0.0f;
    // cv2.solvePnPRansac's final solvePnP (also its five-candidate shortcut), not plain cv2.solvePnP; MR_EPNP_CV_EARLY_RETURN: exactly five
    // candidates take OpenCV >= 3.3's early return — solvePnP(EPNP) on the float32 inputs (oracle/epnp.inc decision (ii))
    const bool use_ransac_refit_f64 = cv.ransac_thr != nullptr && !(a.flags & MR_EPNP_REFIT_F32) &&
                                      !((a.flags & MR_EPNP_CV_EARLY_RETURN) && mode == EP_MODE_PLAIN && n == 5);
    auto fetch = [&](int q, float (&o)[3], float (&im)[2]) {          // point index -> float32 correspondence
        typename GeoTile<T>::Raw r;
        tl.load(q, r);
        o[0] = (float)to_f(r.x); o[1] = (float)to_f(r.y); o[2] = (float)to_f(r.z); im[0] = (float)to_f(r.u); im[1] = (float)to_f(r.v);
    };
    const uint16_t *list = slist;
    int n_fit = n, iters_run = 0, best = 0, besth = -1;
    bool ok = true;
    if (mode == EP_MODE_RANSAC) {
        // the loop's state: fresh in round 0, where round 0 left it in round 1
        int niters = ea.max_iters > 1 ? ea.max_iters : 1;
        if (ea.h0 > 0) { niters = meta[EP_M_NITERS]; best = meta[EP_M_BEST]; besth = meta[EP_M_BESTH]; }
        const int hend = ea.h1 < niters ? ea.h1 : niters;     // hypotheses at or beyond the loop's bound were not solved: nothing can reach them
        static_assert(kEpMaxIters <= NT, "one thread per hypothesis record");
        if (tid < kEpMaxIters && ((tid >= ea.h0 && tid < hend) || tid == besth)) {            // this round's hypotheses (+ the best model so far: its mask may be needed)
            // R (through the Rodrigues round trip of solvePnP's output) | t of the hypothesis' best candidate, as the hypothesis launch left it
            const long long nq = ea.w.nq, q = (long long)b * kEpMaxIters + tid;
#pragma unroll
            for (int i = 0; i < 12; ++i) shyp[tid * 12 + i] = ea.w.hrt[i * nq + q];
        }
        for (int i = tid; i < 4 * 32; i += NT) scnt[i] = 0;
        for (int i = tid; i < (P + 31) >> 5; i += NT) smask[i] = 0u;
        __syncthreads();
        EPC_STAMP(1);

        // ---- consensus of every hypothesis over the candidates
        const float thr2 = (float)((double)thr_given * (double)thr_given);
        const int nct = (n + NT - 1) / NT;
        const int nlc = (n + 63) >> 6;
        // a round of few hypotheses keeps every ballot: chunk (i0 + k) * WPO + wid holds the candidates 64 chunk ... + 63, the numbering of the list compaction below
        const bool keep_ballots = ea.h1 - ea.h0 <= kEpKeptBallots;
        for (int i0 = 0; i0 < nct; i0 += 4) {
            float po[4][3], pi[4][2];
            bool lv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qi = (i0 + k) * NT + tid;
                lv[k] = (i0 + k < nct) && qi < n;
                fetch((int)slist[lv[k] ? qi : 0], po[k], pi[k]);
            }
            for (int h = ea.h0; h < hend; ++h) {
                double R[9], t[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = shyp[h * 12 + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) t[i] = shyp[h * 12 + 9 + i];
                int c = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned long long bal = __ballot(lv[k] && ep_is_inlier(cam, R, t, po[k][0], po[k][1], po[k][2], pi[k][0], pi[k][1], thr2));
                    c += __popcll(bal);
                    if (keep_ballots && lane == 0 && (i0 + k) * WPO + wid < nlc) sbal_h[(h - ea.h0) * a.nca + (i0 + k) * WPO + wid] = bal;
                }
                if (lane == 0) scnt[wid * 32 + h] += c;
            }
        }
        __syncthreads();
        EPC_STAMP(2);

        // ---- RANSAC's loop replayed over the counts, in RNG order (ptsetreg.cpp run), as far as this round's hypotheses reach
        // (by wave 0 alone, its state through LDS: RANSACUpdateNumIters is a pow and two logs of the device math library — ~600
        //  instructions per accepted model that all four waves used to execute, 2.4 M of the launch's 13 M)
        int it = ea.h0;
        if (wid == 0) {
            for (; it < niters && it < ea.h1; ++it) {
                const int good = scnt[it] + scnt[32 + it] + scnt[64 + it] + scnt[96 + it];
                if (good > (best > 4 ? best : 4)) {
                    best = good; besth = it;
                    niters = ep_update_iters(0.99, (double)(n - good) / n, 5, niters);
                }
            }
            if (lane == 0) { scnt[128] = it; scnt[129] = niters; scnt[130] = best; scnt[131] = besth; }
        }
        __syncthreads();
        it = scnt[128]; niters = scnt[129]; best = scnt[130]; besth = scnt[131];
        iters_run = it;
        EPC_STAMP(3);
        if (it < niters && ea.h1 < kEpMaxIters) {                  // the loop goes on: the remaining hypotheses are solved in the next round
            if (tid == 0) { meta[EP_M_PENDING] = 1; meta[EP_M_NITERS] = niters; meta[EP_M_BEST] = best; meta[EP_M_BESTH] = besth; meta[EP_M_ITERS] = it; }
            // ... on the samples of the hypotheses [h1, niters), which the front launch left to this one: their correspondences from the
            // tile (the float32 values ep_fetch_global returns) -> the workspace's sample records, as the front launch writes [0, h1)
            const uint16_t *spt = ea.w.spt + (long long)b * (5 * kEpMaxIters);
            for (int k = 5 * ea.h1 + tid; k < 5 * niters; k += NT) {
                const int h = k / 5, i = k - 5 * h;
                float o[3], im[2];
                fetch((int)spt[k], o, im);
                float *s = ea.w.samp + ((long long)b * kEpMaxIters + h) * kEpSampRec + 5 * i;
                s[0] = o[0]; s[1] = o[1]; s[2] = o[2]; s[3] = im[0]; s[4] = im[1];
            }
            EPC_STAMP(7); EPC_STAMP(9);
            return;
        }
        if (best <= 0) ok = false;
        else {
            // ---- inliers of the best model: mask in point space, compacted list (ascending)
            // the best model was counted in THIS round and its ballots were kept: they are these bits (the same predicate on the same operands).  Otherwise
            // (the first round's best model in the second round, a round wider than kEpKeptBallots) the test is evaluated again
            const bool kept = keep_ballots && besth >= ea.h0 && besth < hend;
            const unsigned long long *bl = kept ? sbal_h + (besth - ea.h0) * a.nca : sball;
            if (!kept) {
                double R[9], t[3];
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = shyp[besth * 12 + i];
#pragma unroll
                for (int i = 0; i < 3; ++i) t[i] = shyp[besth * 12 + 9 + i];
                for (int i = 0; i < nct; ++i) {
                    const int qi = i * NT + tid;
                    const bool lvq = qi < n;
                    const int pidx = slist[lvq ? qi : 0];
                    float o[3], im[2];
                    fetch(pidx, o, im);
                    const bool in = lvq && ep_is_inlier(cam, R, t, o[0], o[1], o[2], im[0], im[1], thr2);
                    const unsigned long long bal = __ballot(in);
                    if (lane == 0 && i * WPO + wid < nlc) sball[i * WPO + wid] = bal;
                }
                __syncthreads();
            }
            int ex0, ex1;
            n_fit = scan_chunks(bl, nlc, lane, ex0, ex1);
            for (int i = 0; i < nct; ++i) {
                const int chunk = i * WPO + wid;
                if (chunk >= nlc) break;
                const unsigned long long bal = bl[chunk];
                const int base = chunk_base(chunk, ex0, ex1);
                if ((bal >> lane) & 1ull) {
                    const int pidx = slist[chunk * 64 + lane];
                    slist2[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)pidx;
                    atomicOr(&smask[pidx >> 5], 1u << (pidx & 31));
                }
            }
            list = slist2;
            __syncthreads();
        }
    } else {
        // no loop: the list is the candidate list, and its mask (the bit row below) is built here from it — every thread sets the bits of the entries it loaded
        for (int i = tid; i < (P + 31) >> 5; i += NT) smask[i] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += NT) { const int pidx = slist[i]; atomicOr(&smask[pidx >> 5], 1u << (pidx & 31)); }
        __syncthreads();
    }
    EPC_STAMP(4);

    if (ok) {
        // ---- EPnP on the whole set (the re-fit on the inliers, or plain solvePnP): A) centroid, covariance -> control points,
        //      barycentric transform (every lane, identical values)
        const int nn = n_fit;
        const double dn = (double)nn;
        double *sprep = shyp;                             // [21] control points + inverse basis: wave 0 computes, every wave reads (the hypotheses are done with)
        const long long B = a.B;
        if (wid == 0) {
            double cws[4][3], ci[9];
            double s3[3] = { 0.0, 0.0, 0.0 };
            for (int i = lane; i < nn; i += 64) { float o[3], im[2]; fetch((int)list[i], o, im); s3[0] += (double)o[0]; s3[1] += (double)o[1]; s3[2] += (double)o[2]; }
            wave_allreduce<3>(s3);
#pragma unroll
            for (int j = 0; j < 3; ++j) cws[0][j] = s3[j] / dn;
            double s6[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
            for (int i = lane; i < nn; i += 64) {
                float o[3], im[2]; fetch((int)list[i], o, im);
                const double q[3] = { (double)o[0] - cws[0][0], (double)o[1] - cws[0][1], (double)o[2] - cws[0][2] };
                s6[0] = fma(q[0], q[0], s6[0]); s6[1] = fma(q[0], q[1], s6[1]); s6[2] = fma(q[0], q[2], s6[2]);
                s6[3] = fma(q[1], q[1], s6[3]); s6[4] = fma(q[1], q[2], s6[4]); s6[5] = fma(q[2], q[2], s6[5]);
            }
            wave_allreduce<6>(s6);
            const double C[9] = { s6[0], s6[1], s6[2], s6[1], s6[3], s6[4], s6[2], s6[4], s6[5] };
            double dc[3], uct[9];
            ep_eig3(C, dc, uct);
            double kv[3];
#pragma unroll
            for (int i = 1; i < 4; ++i) {
                const double kk = sqrt((dc[i - 1] > 0.0 ? dc[i - 1] : 0.0) / dn);
                kv[i - 1] = kk;
#pragma unroll
                for (int j = 0; j < 3; ++j) cws[i][j] = cws[0][j] + kk * uct[3 * (i - 1) + j];
            }
            ep_basis_pinv(kv, uct, ci);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) { sprep[3 * i + j] = cws[i][j]; ea.w.prep_r[(long long)b * 24 + (3 * i + j)] = cws[i][j]; }
#pragma unroll
                for (int i = 0; i < 9; ++i) { sprep[12 + i] = ci[i]; ea.w.prep_r[(long long)b * 24 + (12 + i)] = ci[i]; }
            }
        } else {
            // ... while the other waves, which have nothing to do until the control points exist, store what depends on none of it: the inlier mask
            // in point space and the re-fit's list
            const int t = tid - 64;
            if (mode == EP_MODE_RANSAC)
                for (int p = t; p < P; p += NT - 64) cv.init_mask[(long long)b * P + p] = (uint8_t)((smask[p >> 5] >> (p & 31)) & 1u);
            for (int i = t; i < nn; i += NT - 64) ea.w.fit[(long long)b * ea.w.pstride + i] = list[i];
            // ... and the list once more as a mask, one bit per point: what the LM launch that carries the re-fit keeps in LDS beside the list
            // (it used to rebuild both from init_mask's bytes)
            const int nw32 = (P + 31) >> 5;
            const int nw64 = ep_fitbits_stride(P);
            unsigned long long *const bits = ep_fitbits(ea.w, a.B) + (long long)b * nw64;
            for (int c = t; c < nw64; c += NT - 64)
                bits[c] = (unsigned long long)smask[2 * c] | ((unsigned long long)(2 * c + 1 < nw32 ? smask[2 * c + 1] : 0u) << 32);
        }
        __syncthreads();
        EPC_STAMP(5);

        // what every point needs of the above is wave-uniform: into scalar registers (the accumulators below want the vector ones)
        double cws[4][3], ci[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) { cws[0][j] = uni(sprep[j]); cws[1][j] = cws[2][j] = cws[3][j] = 0.0; }
#pragma unroll
        for (int i = 0; i < 9; ++i) ci[i] = uni(sprep[12 + i]);
        EpCam camu;
        camu.fx = uni(cam.fx); camu.fy = uni(cam.fy); camu.cx = uni(cam.cx); camu.cy = uni(cam.cy);
        const EpRefitPoint<T, GeoTile<T>> point{ tl, list, camu, cws, ci, uni(1.0 / cam.fx), uni(1.0 / cam.fy), use_ransac_refit_f64 };
        // B) M^T M: wave w owns the entries k = w mod 4 of the upper triangle
        double acc[12], ext[5], afirst[4];
        const double pw0[3] = { cws[0][0], cws[0][1], cws[0][2] };
#define EP_MTM_DO(W_) do { ep_mtm_part<W_, T>(point, camu, pw0, nn, lane, acc, ext, afirst); \
                          if (lane == 0) { ep_mtm_store<W_>(acc, camu, ea.w.mtm_r, B, b); ep_abt_store<W_>(ext, afirst, ea.w.abt_r, B, b); } } while (0)
        static_assert(WPO == 4, "one M^T M part per wave");
        if (wid == 0) EP_MTM_DO(0); else if (wid == 1) EP_MTM_DO(1); else if (wid == 2) EP_MTM_DO(2); else EP_MTM_DO(3);
#undef EP_MTM_DO
        EPC_STAMP(6);
    }
    if (tid == 0) { meta[EP_M_NFIT] = n_fit; meta[EP_M_REFIT] = ok ? (use_ransac_refit_f64 ? 3 : 1) : 0; meta[EP_M_ITERS] = iters_run; meta[EP_M_BEST] = best; meta[EP_M_BESTH] = besth; }
    EPC_STAMP(7); EPC_STAMP(9);
