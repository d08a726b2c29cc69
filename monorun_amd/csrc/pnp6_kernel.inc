// pnp6_kernel.inc — true 6-DoF refinement (SURVEY.md §8f row N4: "a true 6-DoF option (use_6dof)"; the north-star's "6x6
// J^T Sigma^-1 J normal-equation build and solve").  The reference accepts `use_6dof` and ignores it (pnp_uncert.py:11), so
// there is no reference code for this variant: it is the SAME residual functor as the 4-DoF solver
// (pnp_uncert_cpu.cpp:24-51: rotate, translate, z clamp, project, u/v clamps, weight) with the full angle-axis vector
// r = (rx, ry, rz) in ceres::AngleAxisRotatePoint instead of (0, yaw, 0), pose6 = [rx, ry, rz, tx, ty, tz], the same
// Ceres-1.14 trust-region LM, and covariance = (J^T J)^-1 with the solver's Jacobian.  It starts from the 4-DoF result
// (r = (0, yaw, 0), t) on that solve's final inlier set: mr_pnp6_refine_batched is the second launch of
// pnp_uncert(..., use_6dof=True).
//
// One workgroup of 4 wavefronts per object; point records in LDS (same tile as the 4-DoF kernel); the Jacobian in closed
// form: d(R(r) X)/dr = -[R X]x J_l(r) (left Jacobian of SO(3)), which is what Ceres' Jets produce for the Rodrigues
// branch, and d(X + r x X)/dr = -[X]x in the first-order branch it takes for |r|^2 <= eps.  28 block sums per
// evaluation (21 of the upper triangle of J^T J, 6 of J^T r, the cost), reduced with the same permlane / DPP tree.

struct Pnp6Args {
    const void *x2d, *istd, *x3d;
    long long s2[3], sw[3], s3[3];
    int vec, elem_size;
    const void *K; int K_stride; int K_f64;
    const void *ur, *vr; int r_stride; int r_f64;
    const uint8_t *mask; const float *pose4; const uint8_t *valid4;
    int B, P; double z_min; int lm_max_iter; int from_head;     // from_head: always 0 (field shared with load_records)
    uint8_t *valid; float *pose6; float *cov6; float *diag;
};

#ifndef MR_PNP6_WAVES
#define MR_PNP6_WAVES 3
#endif
constexpr int kAcc6 = 28;
constexpr int kWpo6 = 4, kThreads6 = 64 * kWpo6;      // waves per object.  Measured (1024 config-2 objects, tools/gpu_pnp6_time.py): 4 waves 105 us (two rounds of
                                                      // workgroups at 219 VGPRs; 512 objects = one round: 61 us), 2 waves 102 us (one round, passes twice as long), 4 waves
                                                      // forced to 168 / 128 VGPRs by launch bounds 137 / 176 us (spills).  The 17-iteration object ALONE on the GPU takes
                                                      // 69 us (2-iteration object: 26 us; ~3.0 us per pass): the launch is its slowest chain AND two rounds of bulk.
                                                      // Round 3: covariance from the LM's own H (x == out at every exit: one evaluation less), one factorisation for
                                                      // the six right-hand sides, by wave 0 only: 105.6 -> 99.1 us, outputs bit-identical.
                                                      // Tried and not kept: the 4-DoF kernel's
                                                      // leader / follower protocol with the totals in LDS — one round of workgroups at 128 VGPRs, 94.4 us, but a longer
                                                      // pass (2.8 -> 3.2 - 3.5 us): slower for one image's ~100 objects, where the launch is its slowest object.
                                                      // Round 5: the LM's H / g lane-packed (Eval6), the rotation, the iterate and the scaling in scalar registers:
                                                      // 219 VGPRs + 104 SGPR spills -> 163 + 58, three waves per SIMD without scratch; 99.1 -> 89.9 us per 1024 objects,
                                                      // the 17-iteration object alone 69 -> 65 us (outputs unchanged).
__device__ __forceinline__ constexpr int tri6(int i, int j) { return tri_index<6>(i, j); }        // packed upper triangle, row-major

struct Rot6 { double R[9]; double D[9]; bool small; };             // D: columns j_k of J_l(r) (row-major 3x3), unused when small

__device__ __forceinline__ void rot6_setup(const double (&x)[6], Rot6 &q) {
    const double rx = x[0], ry = x[1], rz = x[2];
    const double th2 = rx * rx + ry * ry + rz * rz;
    q.small = !(th2 > 2.220446049250313e-16);
    if (q.small) {                                                  // R X ~ X + r x X  (rotation.h first-order branch)
        q.R[0] = 1.0; q.R[1] = -rz; q.R[2] = ry; q.R[3] = rz; q.R[4] = 1.0; q.R[5] = -rx; q.R[6] = -ry; q.R[7] = rx; q.R[8] = 1.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) q.D[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double ith = fast_rsqrt(th2), th = th2 * ith;
    double sn, cs;
    fast_sincos(th, sn, cs);
    const double ax = rx * ith, ay = ry * ith, az = rz * ith, c1 = 1.0 - cs;
    q.R[0] = cs + c1 * ax * ax;      q.R[1] = c1 * ax * ay - sn * az; q.R[2] = c1 * ax * az + sn * ay;
    q.R[3] = c1 * ax * ay + sn * az; q.R[4] = cs + c1 * ay * ay;      q.R[5] = c1 * ay * az - sn * ax;
    q.R[6] = c1 * ax * az - sn * ay; q.R[7] = c1 * ay * az + sn * ax; q.R[8] = cs + c1 * az * az;
    const double sa = sn * ith, sb = 1.0 - sa, sc = c1 * ith;       // J_l = sa I + sb a a^T + sc [a]x
    q.D[0] = sa + sb * ax * ax;      q.D[1] = sb * ax * ay - sc * az; q.D[2] = sb * ax * az + sc * ay;
    q.D[3] = sb * ax * ay + sc * az; q.D[4] = sa + sb * ay * ay;      q.D[5] = sb * ay * az - sc * ax;
    q.D[6] = sb * ax * az - sc * ay; q.D[7] = sb * ay * az + sc * ax; q.D[8] = sa + sb * az * az;
}

// cost, gradient and packed upper triangle of J^T J at x over the listed points (every thread returns the same totals)
// The 28 totals come back LANE-PACKED (lane t < 28 of every wave holds total t: 0..20 the upper triangle of J^T J, 21..26 J^T r, 27 the
// sum of squares) — the LM keeps two such registers (the iterate's and the candidate's) instead of two sets of 27 wave-uniform doubles
// in every lane, and reads the entries it needs with v_readlane (round 5: 219 -> see profiles/r05_kernel_resources.txt).
struct Eval6 { double v; double cost; bool ok; };
__device__ __forceinline__ double h6(const Eval6 &e, int i, int j) { return readlane_d(e.v, tri6(i, j)); }
__device__ __forceinline__ double g6(const Eval6 &e, int j) { return readlane_d(e.v, 21 + j); }

template <typename T>
__device__ void eval6(const Cam &k, const double (&x)[6], const uint16_t *list, int n, const Tile<T> &tl, double *red, int &flip, Eval6 &out) {
    Rot6 q;
    rot6_setup(x, q);
    // wave-uniform: into scalar registers (the 28 accumulators and the point's temporaries want the vector ones)
#pragma unroll
    for (int i = 0; i < 9; ++i) { q.R[i] = uni(q.R[i]); q.D[i] = uni(q.D[i]); }
    const double x3 = uni(x[3]), x4 = uni(x[4]), x5 = uni(x[5]);
    double acc[kAcc6];
#pragma unroll
    for (int i = 0; i < kAcc6; ++i) acc[i] = 0.0;
    for (int i = threadIdx.x; i < n; i += kThreads6) {
        typename Tile<T>::Raw ra;
        tl.load((int)list[i], ra);
        const double X = (double)to_f(ra.x), Y = (double)to_f(ra.y), Z = (double)to_f(ra.z);
        const double wu = (double)to_f(ra.wu), wv = (double)to_f(ra.wv);
        const double Yx = q.R[0] * X + q.R[1] * Y + q.R[2] * Z, Yy = q.R[3] * X + q.R[4] * Y + q.R[5] * Z, Yz = q.R[6] * X + q.R[7] * Y + q.R[8] * Z;
        const double Xc = Yx + x3, Yc = Yy + x4, Zc = Yz + x5;
        const bool zc = Zc < k.zmin;
        const double Zu = zc ? k.zmin : Zc;
        const double iz = fast_rcp(Zu);
        const double px = k.fx * Xc * iz, py = k.fy * Yc * iz;
        double pu = px + k.cx, pv = py + k.cy;
        const bool ucl = (pu < k.umin) || (pu > k.umax), vcl = (pv < k.vmin) || (pv > k.vmax);
        pu = fmin(fmax(pu, k.umin), k.umax); pv = fmin(fmax(pv, k.vmin), k.vmax);
        const double ru = wu * (pu - (double)to_f(ra.u)), rv = wv * (pv - (double)to_f(ra.v));
        // rows of d(proj)/d(Xc): (fx/z, 0, -px/z) and (0, fy/z, -py/z); a clamped z is a constant, a clamped u / v a constant row
        const double wuz = ucl ? 0.0 : wu * iz, wvz = vcl ? 0.0 : wv * iz;
        const double aux = wuz * k.fx, auz = zc ? 0.0 : -wuz * px;
        const double avy = wvz * k.fy, avz = zc ? 0.0 : -wvz * py;
        // rotation columns: d(Xc)/d r_k = j_k x (R X)   (first-order branch: e_k x X)
        const double bx = q.small ? X : Yx, by = q.small ? Y : Yy, bz = q.small ? Z : Yz;
        double Ju[6], Jv[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double jx = q.D[c], jy = q.D[3 + c], jz = q.D[6 + c];      // column c of J_l
            const double dx = jy * bz - jz * by, dy = jz * bx - jx * bz, dz = jx * by - jy * bx;
            Ju[c] = aux * dx + auz * dz;
            Jv[c] = avy * dy + avz * dz;
        }
        Ju[3] = aux; Ju[4] = 0.0; Ju[5] = auz;
        Jv[3] = 0.0; Jv[4] = avy; Jv[5] = avz;
        int t = 0;
#pragma unroll
        for (int m = 0; m < 6; ++m) {
#pragma unroll
            for (int nn = m; nn < 6; ++nn, ++t) acc[t] = fma(Ju[m], Ju[nn], fma(Jv[m], Jv[nn], acc[t]));
            acc[21 + m] = fma(Ju[m], ru, fma(Jv[m], rv, acc[21 + m]));
        }
        acc[27] = fma(ru, ru, fma(rv, rv, acc[27]));
    }
    out.v = block_sum_packed<kWpo6, kAcc6>(acc, red, flip);
    out.cost = 0.5 * readlane_d(out.v, 27);
    out.ok = __builtin_amdgcn_ballot_w64(((int)threadIdx.x & 63) < kAcc6 && !isfinite(out.v)) == 0ull && isfinite(out.cost);
}

template <typename T>
__global__ void __launch_bounds__(kThreads6, MR_PNP6_WAVES) pnp6_refine_kernel(const Pnp6Args a) {
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = a.P, nchunk = (P + 63) >> 6;
    extern __shared__ __align__(16) unsigned char smem[];
    double *red = (double *)smem;                                           // [2][4][kRedN]
    unsigned long long *sball = (unsigned long long *)(red + 2 * 4 * kRedN);  // [nchunk rounded to 4]   (the scratch keeps its four-wave size)
    unsigned char *tile_base = (unsigned char *)(sball + ((nchunk + 3) & ~3));
    Tile<T> tl;
    tl.ra = (const T *)tile_base; tl.rb = (const T *)tile_base + (size_t)4 * P;
    uint16_t *slist = (uint16_t *)(tile_base + (size_t)8 * P * sizeof(T));
    int flip = 0;

    load_records<T, Pnp6Args>(a, b, P, kThreads6, tl);
    // inlier list from the 4-DoF solve's mask (ascending point order), built like the candidate list of the 4-DoF kernel
    const int npt = (P + kThreads6 - 1) / kThreads6;
    for (int i = 0; i < npt; ++i) {
        const int p = i * kThreads6 + tid;
        const bool in = (p < P) && a.mask[(long long)b * P + (p < P ? p : 0)] != 0;
        const unsigned long long bal = __ballot(in);
        if (lane == 0 && i * kWpo6 + wid < nchunk) sball[i * kWpo6 + wid] = bal;
    }
    __syncthreads();
    int ex0, ex1;
    const int n = scan_chunks(sball, nchunk, lane, ex0, ex1);
    for (int i = 0; i < npt; ++i) {
        const int chunk = i * kWpo6 + wid;
        if (chunk >= nchunk) break;
        const unsigned long long bal = sball[chunk];
        const int base = chunk_base(chunk, ex0, ex1);
        if ((bal >> lane) & 1ull) slist[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)(chunk * 64 + lane);
    }
    __syncthreads();

    const long long ko = (long long)b * a.K_stride, ro = (long long)b * a.r_stride;
    Cam cam;
    cam.fx = uni(ld_k(a.K, a.K_f64, ko + 0)); cam.fy = uni(ld_k(a.K, a.K_f64, ko + 4));
    cam.cx = uni(ld_k(a.K, a.K_f64, ko + 2)); cam.cy = uni(ld_k(a.K, a.K_f64, ko + 5));
    cam.zmin = uni(a.z_min);
    cam.umin = uni(ld_k(a.ur, a.r_f64, ro)); cam.umax = uni(ld_k(a.ur, a.r_f64, ro + 1));
    cam.vmin = uni(ld_k(a.vr, a.r_f64, ro)); cam.vmax = uni(ld_k(a.vr, a.r_f64, ro + 1));

    const int N = 6;
    const bool have4 = a.valid4[b] != 0, start_ok = have4 && n > 0;
    // (the iterate, the returned pose and the Jacobi scaling are wave-uniform: scalar registers)
    double x[6] = { 0.0, uni((double)a.pose4[(long long)b * 4]), 0.0, uni((double)a.pose4[(long long)b * 4 + 1]), uni((double)a.pose4[(long long)b * 4 + 2]),
                    uni((double)a.pose4[(long long)b * 4 + 3]) };
    double out[6];
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = x[j];
    Eval6 cur;
    cur.v = 0.0; cur.cost = 0.0; cur.ok = false;
    bool ok = false, usable = false;
    double radius = 1e4, decrease_factor = 2.0;
    int iteration = 0, why = WHY_K0FAIL;
    if (start_ok) {
        eval6<T>(cam, x, slist, n, tl, red, flip, cur);
        ok = cur.ok;
        why = WHY_EVALFAIL;
    }
    if (start_ok && ok) {
        // Ceres 1.14 TrustRegionMinimizer + LevenbergMarquardtStrategy, the flow of lm_solve (pnp_kernel.inc) for 6 parameters
        double scale[6];
#pragma unroll
        for (int j = 0; j < N; ++j) { const double h = h6(cur, j, j); scale[j] = uni(fast_rcp(1.0 + (h > 0.0 ? h * fast_rsqrt(h) : 0.0))); }
        double x_norm = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) x_norm += x[j] * x[j];
        x_norm = sqrt(x_norm);
        bool last_successful = true;
        int invalid_run = 0;
        for (;;) {
            if (last_successful) {
#pragma unroll
                for (int j = 0; j < N; ++j) out[j] = x[j];
            }
            if (iteration >= a.lm_max_iter) { why = WHY_MAXITER; usable = true; break; }
            if (last_successful) {
                double gmax = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) gmax = fmax(gmax, fabs(g6(cur, j)));
                if (gmax <= 1e-10) { why = WHY_GRADIENT; usable = true; break; }
            }
            if (radius <= 1e-32) { why = WHY_MINRADIUS; usable = true; break; }
            ++iteration; last_successful = false;
            double A[36], gs[6], y[6], delta[6];
#pragma unroll
            for (int m = 0; m < N; ++m) {
                gs[m] = g6(cur, m) * scale[m];
#pragma unroll
                for (int nn = 0; nn < N; ++nn) A[6 * m + nn] = h6(cur, m, nn) * scale[m] * scale[nn];
            }
            const double inv_radius = fast_rcp(radius);
#pragma unroll
            for (int j = 0; j < N; ++j) A[7 * j] += fmin(fmax(A[7 * j], 1e-6), 1e32) * inv_radius;
            bool step_ok = chol_solve_fast<6>(A, gs, y);
            double dg = 0.0, dHd = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) { delta[j] = -y[j] * scale[j]; step_ok = step_ok && isfinite(delta[j]); }
#pragma unroll
            for (int m = 0; m < N; ++m) {
                dg = fma(delta[m], g6(cur, m), dg);
                double t = 0.0;
#pragma unroll
                for (int nn = 0; nn < N; ++nn) t = fma(h6(cur, m, nn), delta[nn], t);
                dHd = fma(delta[m], t, dHd);
            }
            const double model_cost_change = -(dg + 0.5 * dHd);
            step_ok = step_ok && (model_cost_change > 0.0);
            if (!step_ok) {
                if (++invalid_run >= 5) { why = WHY_INVALID; usable = false; break; }
                radius *= 0.5;
                continue;
            }
            invalid_run = 0;
            double cand[6];
#pragma unroll
            for (int j = 0; j < N; ++j) cand[j] = x[j] + delta[j];
            Eval6 ce;
            eval6<T>(cam, cand, slist, n, tl, red, flip, ce);
            double ccost = ce.cost;
            if (!ce.ok) ccost = 1.7976931348623157e308;
            double step_norm = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) { const double d = x[j] - cand[j]; step_norm += d * d; }
            step_norm = sqrt(step_norm);
            if (step_norm <= 1e-8 * (x_norm + 1e-8)) { why = WHY_PARAMETER; usable = true; break; }
            const double cost_change = cur.cost - ccost;
            if (fabs(cost_change) <= 1e-6 * cur.cost) { why = WHY_FUNCTION; usable = true; break; }
            const double rd = cost_change * fast_rcp(model_cost_change);
            if (rd > 1e-3) {
                x_norm = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) { x[j] = uni(cand[j]); x_norm += x[j] * x[j]; }
                x_norm = sqrt(x_norm);
                cur.v = ce.v; cur.cost = ccost;
                last_successful = true;
                const double t = 2.0 * rd - 1.0;
                radius = fmin(1e16, radius * fast_rcp(fmax(1.0 / 3.0, 1.0 - t * t * t)));
                decrease_factor = 2.0;
            } else {
                radius = radius * fast_rcp(decrease_factor); decrease_factor *= 2.0;
            }
        }
    }
    // covariance = (J^T J)^-1 at the returned pose (solver Jacobian)
    bool valid = start_ok && ok && usable;
    double cov[36];
#pragma unroll
    for (int i = 0; i < 36; ++i) cov[i] = (i % 7 == 0) ? 1.0 : 0.0;
    if (wid != 0) return;                               // outputs are wave 0's business: the other waves free their SIMD slots
    if (valid) {
        // the LM leaves x == out at every exit (x moves only when a step is accepted, and `out` follows at the top of the next
        // pass; the tolerance exits leave before the candidate is taken), so H IS J^T J at the returned pose: no further evaluation.
        // One factorisation, six pairs of substitutions (the same operations chol_solve_fast performs for every right-hand side).
        double A[36], L[36], inv[6];
#pragma unroll
        for (int m = 0; m < N; ++m)
#pragma unroll
            for (int nn = 0; nn < N; ++nn) A[6 * m + nn] = h6(cur, m, nn);
        bool inv_ok = chol_factor_fast<6>(A, L, inv) && 2 * n >= N;      // 2 n < 6 residuals: J^T J is singular, whichever way a rounding-level pivot falls
#pragma unroll
        for (int c = 0; c < N; ++c) {
            double e[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, s[6];
            e[c] = 1.0;
            chol_substitute<6>(L, inv, e, s);
#pragma unroll
            for (int r = 0; r < N; ++r) { cov[6 * r + c] = s[r]; inv_ok = inv_ok && isfinite(s[r]); }
        }
        if (!inv_ok) {
            valid = false;
#pragma unroll
            for (int i = 0; i < 36; ++i) cov[i] = (i % 7 == 0) ? 1.0 : 0.0;
        }
    }
    if (tid == 0) {
        a.valid[b] = valid ? 1 : 0;
#pragma unroll
        for (int j = 0; j < N; ++j) a.pose6[(long long)b * 6 + j] = have4 ? (float)out[j] : 0.0f;      // the start pose unless the LM moved it; zeros only without a 4-DoF result
        if (a.diag) { a.diag[(long long)b * 2] = (float)iteration; a.diag[(long long)b * 2 + 1] = (float)why; }
#pragma unroll
        for (int i = 0; i < 36; ++i) a.cov6[(long long)b * 36 + i] = (float)cov[i];
    }
}
