// pnp_noc_kernel.inc — the two 7-parameter variants of the reference's C ABI (SURVEY.md §8f, row N4):
// pnp_noc_uncert / pnp_noc_cov_uncert (src/ext.h:15-43, pnp_uncert_cpu.cpp:294-377).  The reference exports them and never
// calls them from Python.  BATCHED here: one workgroup of 4 wavefronts per object (grid = number of objects), the legacy
// per-object entry points launch a batch of one.
//   dimpose = [log l, log h, log w, yaw, tx, ty, tz]; the NOC point is scaled by exp(log-dims), rotated about y by
//   ceres::AngleAxisRotatePoint((0, yaw, 0)) (both of its branches), translated, z-clamped, projected, u/v-clamped
//   (NocReprojectionErrorArray :98-160); residual = W (proj - x2d) with W = diag(wxx, wyy) or the full symmetric
//   [wxx wxy; wxy wyy] (NocCovReprojectionErrorArray :163-228); a 3-residual prior on the log-dims (DimErrorArray :77-95);
//   EVERY block goes through one ceres::HuberLoss(delta) (:311,:324) — Ceres' Corrector with rho'' <= 0 scales residuals and
//   Jacobian rows by sqrt(rho').
// The Jacobian is written in closed form (what Ceres' Jet<double,7> arithmetic evaluates to, clamp semantics included:
// a clamped quantity is a constant): d(Xc)/d(log-dim k) = (column k of R_y) * pt_k, d(Xc)/d(yaw) = (Zr, 0, -Xr),
// d(Xc)/dt = I, chained with the 2x3 projection rows.  36 block sums per evaluation (28 of the upper triangle of J^T J,
// 7 of J^T r, the robustified cost) land in LDS, where the LM (same Ceres-1.14 flow as the 4-DoF solver) reads them:
// nothing of size 7x7 stays in registers across an evaluation.

struct NocArgs {
    const double *pts2d, *pts3d, *wgt2d, *logdim, *logdim_wgt, *K, *init, *clips;   // per object: (pn,2) (pn,3) (pn,ws) (3) (3) | (9) (7) (5)
    int K_batch, clips_batch;                                                        // 1 = shared by all objects
    double delta; int pn, full_cov, B;
    double *out_dimpose; int *out_val; double *out_diag;                             // (B,7), (B), (B,2) [iterations, final cost] or null
};

constexpr int kNocAcc = 36;
__device__ __forceinline__ constexpr int tri7(int i, int j) { return tri_index<7>(i, j); }        // packed upper triangle, row-major, i <= j after ordering

// In-place Cholesky solve of a packed symmetric positive definite N x N system (upper triangle, tri-index order): the
// factor overwrites `A`, so N(N+1)/2 doubles are live instead of 2 N^2.  Reciprocal pivots from v_rsq_f64 (fast_rsqrt).
template <int N>
__device__ __forceinline__ bool chol_packed_solve(double (&A)[N * (N + 1) / 2], const double (&b)[N], double (&x)[N]) {
    auto idx = [](int i, int j) constexpr { const int a = i <= j ? i : j, c = i <= j ? j : i; return a * N - a * (a - 1) / 2 + (c - a); };
    double inv[N];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {                       // A holds U with A = U^T U (row j of U in the packed row j)
        double s = A[idx(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) s = fma(-A[idx(k, j)], A[idx(k, j)], s);
        if (!(s > 0.0) || !isfinite(s)) ok = false;
        const double r = fast_rsqrt(s);
        inv[j] = r; A[idx(j, j)] = s * r;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double t = A[idx(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) t = fma(-A[idx(k, j)], A[idx(k, i)], t);
            A[idx(j, i)] = t * r;
        }
    }
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = fma(-A[idx(k, i)], y[k], s);
        y[i] = s * inv[i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s = fma(-A[idx(i, k)], x[k], s);
        x[i] = s * inv[i];
    }
    return ok;
}

// ceres::HuberLoss + Corrector (rho'' <= 0 branch) on one residual block: returns sqrt(rho') and adds rho/2 to `cost`
__device__ __forceinline__ double huber_scale(double delta, double s, double &cost_acc) {
    const double b = delta * delta;
    double rho0 = s, rho1 = 1.0;
    if (s > b) { const double q = sqrt(s); rho0 = 2.0 * delta * q - b; rho1 = fmax(2.2250738585072014e-308, delta / q); }
    cost_acc += 0.5 * rho0;
    return sqrt(rho1);
}

// the 36 robustified block sums at x -> LDS `out` (every thread may read them after the call); returns false on a non-finite sum
__device__ bool noc_evaluate(const NocArgs &a, int b, const double (&x)[7], double *red, int &flip, double *out) {
    const double *K = a.K + (a.K_batch == 1 ? 0 : (long long)b * 9), *cl = a.clips + (a.clips_batch == 1 ? 0 : (long long)b * 5);
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double zmin = cl[0], umin = cl[1], umax = cl[2], vmin = cl[3], vmax = cl[4];
    const int ws = a.full_cov ? 3 : 2;
    const double *p2 = a.pts2d + (long long)b * a.pn * 2, *p3 = a.pts3d + (long long)b * a.pn * 3, *pw = a.wgt2d + (long long)b * a.pn * ws;
    const double e0 = exp(x[0]), e1 = exp(x[1]), e2 = exp(x[2]), yaw = x[3];
    const bool small = !(yaw * yaw > 2.220446049250313e-16);             // AngleAxisRotatePoint's first-order branch
    double sn = yaw, cs = 1.0;
    if (!small) fast_sincos(yaw, sn, cs);
    // wave-uniform quantities of the evaluation into scalar registers: the 36 accumulators and the two Jacobian rows want the vector ones
    const double e0u = uni(e0), e1u = uni(e1), e2u = uni(e2), snu = uni(sn), csu = uni(cs), x4 = uni(x[4]), x5 = uni(x[5]), x6 = uni(x[6]);
    double acc[kNocAcc];
#pragma unroll
    for (int i = 0; i < kNocAcc; ++i) acc[i] = 0.0;
    for (int i = threadIdx.x; i < a.pn; i += 256) {
        const double ptx = p3[3 * i] * e0u, pty = p3[3 * i + 1] * e1u, ptz = p3[3 * i + 2] * e2u;
        const double Xr = csu * ptx + snu * ptz, Zr = csu * ptz - snu * ptx;   // small: cs = 1, sn = yaw  ->  x + yaw z, z - yaw x
        const double Xc = Xr + x4, Yc = pty + x5, Zc = Zr + x6;
        const bool zc = Zc < zmin;
        const double Zu = zc ? zmin : Zc, iz = 1.0 / Zu;
        const double px = fx * Xc * iz, py = fy * Yc * iz;
        double pu = px + cx, pv = py + cy;
        const bool ucl = (pu < umin) || (pu > umax), vcl = (pv < vmin) || (pv > vmax);
        pu = ucl ? (pu < umin ? umin : umax) : pu; pv = vcl ? (pv < vmin ? vmin : vmax) : pv;
        const double dx = pu - p2[2 * i], dy = pv - p2[2 * i + 1];
        // d(proj)/d(Xc): u row (fx/z, 0, -px/z), v row (0, fy/z, -py/z); clamped z: third entry 0; clamped u / v: whole row 0
        const double aux = ucl ? 0.0 : fx * iz, auz = (ucl || zc) ? 0.0 : -px * iz;
        const double avy = vcl ? 0.0 : fy * iz, avz = (vcl || zc) ? 0.0 : -py * iz;
        // d(Xc)/d(param): log-dims (columns of R_y times the scaled coordinate), yaw, t
        const double d0x = csu * ptx, d0z = -snu * ptx, d2x = snu * ptz, d2z = csu * ptz;
        const double dyx = small ? ptz : Zr, dyz = small ? -ptx : -Xr;
        double gu[7], gv[7];                                                   // unweighted Jacobian rows of (u, v)
        gu[0] = aux * d0x + auz * d0z; gv[0] = avz * d0z;
        gu[1] = 0.0;                   gv[1] = avy * pty;
        gu[2] = aux * d2x + auz * d2z; gv[2] = avz * d2z;
        gu[3] = aux * dyx + auz * dyz; gv[3] = avz * dyz;
        gu[4] = aux;                   gv[4] = 0.0;
        gu[5] = 0.0;                   gv[5] = avy;
        gu[6] = auz;                   gv[6] = avz;
        double r0, r1, J0[7], J1[7];
        if (a.full_cov) {
            const double wxx = pw[3 * i], wxy = pw[3 * i + 1], wyy = pw[3 * i + 2];
            r0 = wxx * dx + wxy * dy; r1 = wxy * dx + wyy * dy;
#pragma unroll
            for (int k = 0; k < 7; ++k) { J0[k] = wxx * gu[k] + wxy * gv[k]; J1[k] = wxy * gu[k] + wyy * gv[k]; }
        } else {
            const double wxx = pw[2 * i], wyy = pw[2 * i + 1];
            r0 = wxx * dx; r1 = wyy * dy;
#pragma unroll
            for (int k = 0; k < 7; ++k) { J0[k] = wxx * gu[k]; J1[k] = wyy * gv[k]; }
        }
        const double sq = huber_scale(a.delta, r0 * r0 + r1 * r1, acc[35]);
        r0 *= sq; r1 *= sq;
        int q = 0;
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            const double j0 = J0[m] * sq, j1 = J1[m] * sq;
            acc[28 + m] = fma(j0, r0, fma(j1, r1, acc[28 + m]));
#pragma unroll
            for (int n = m; n < 7; ++n, ++q) acc[q] = fma(j0, J0[n] * sq, fma(j1, J1[n] * sq, acc[q]));
        }
    }
    // three packed reductions of 12 sums each: lane k (< 12) of every wave ends up with total 12 c + k, wave 0 parks them in LDS
    // (no broadcast into registers: the LM reads what it needs from `out`)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double part[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) part[i] = acc[12 * c + i];
        const double t = block_sum_packed<4, 12>(part, red, flip);
        if (threadIdx.x < 12) out[12 * c + threadIdx.x] = t;
    }
    __syncthreads();
    // the prior block on the log-dims (DimErrorArray), same loss object: r_k = w_k (x_k - logdim_k), J = diag(w)
    if (threadIdx.x == 0) {
        const double *ld = a.logdim + (long long)b * 3, *lw = a.logdim_wgt + (long long)b * 3;
        double pr[3], s = 0.0, pcost = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pr[k] = lw[k] * (x[k] - ld[k]); s += pr[k] * pr[k]; }
        const double psq = huber_scale(a.delta, s, pcost);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double jk = lw[k] * psq;
            out[tri7(k, k)] += jk * jk;
            out[28 + k] += jk * (pr[k] * psq);
        }
        out[35] += pcost;
    }
    __syncthreads();
    const double v = (threadIdx.x & 63) < kNocAcc ? out[threadIdx.x & 63] : 0.0;
    return __ballot(!isfinite(v)) == 0ull;
}

__global__ void __launch_bounds__(256, 2) pnp_noc_kernel(const NocArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *red = (double *)smem;                      // [2][4][kRedN]
    double *sums = red + 2 * 4 * kRedN;                // [2][40]: block sums of the current iterate / of the candidate
    const int b = blockIdx.x;
    int flip = 0;
    const int N = 7;
    double x[7], out[7];
#pragma unroll
    for (int j = 0; j < N; ++j) { x[j] = a.init[(long long)b * 7 + j]; out[j] = x[j]; }
    int cur = 0;                                       // which half of `sums` holds the current iterate
    double radius = 1e4, decrease_factor = 2.0, cost = 0.0;
    bool usable = false;
    int iteration = 0;
    bool ok = a.pn >= 0 && noc_evaluate(a, b, x, red, flip, sums);
    if (ok) {
        const double *S = sums;
        cost = S[35];
        double scale[7];
#pragma unroll
        for (int j = 0; j < N; ++j) scale[j] = 1.0 / (1.0 + sqrt(S[tri7(j, j)]));
        double x_norm = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) x_norm += x[j] * x[j];
        x_norm = sqrt(x_norm);
        bool last_successful = true;
        int invalid_run = 0;
        for (;;) {
            S = sums + cur * 40;
            if (last_successful) {
#pragma unroll
                for (int j = 0; j < N; ++j) out[j] = x[j];
            }
            if (iteration >= 50) { usable = true; break; }
            if (last_successful) {
                double gmax = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) gmax = fmax(gmax, fabs(S[28 + j]));
                if (gmax <= 1e-10) { usable = true; break; }
            }
            if (radius <= 1e-32) { usable = true; break; }
            ++iteration; last_successful = false;
            double A[28], gs[7], y[7], delta[7];
            {
                int q = 0;
#pragma unroll
                for (int m = 0; m < N; ++m) {
                    gs[m] = S[28 + m] * scale[m];
#pragma unroll
                    for (int n = m; n < N; ++n, ++q) A[q] = S[q] * scale[m] * scale[n];
                }
            }
#pragma unroll
            for (int j = 0; j < N; ++j) A[tri7(j, j)] += fmin(fmax(A[tri7(j, j)], 1e-6), 1e32) / radius;
            bool step_ok = chol_packed_solve<7>(A, gs, y);
            double dg = 0.0, dHd = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) { delta[j] = -y[j] * scale[j]; step_ok = step_ok && isfinite(delta[j]); }
#pragma unroll
            for (int m = 0; m < N; ++m) {
                dg += delta[m] * S[28 + m];
                double t = 0.0;
#pragma unroll
                for (int n = 0; n < N; ++n) t += S[tri7(m, n)] * delta[n];
                dHd += delta[m] * t;
            }
            const double model_cost_change = -(dg + 0.5 * dHd);
            step_ok = step_ok && (model_cost_change > 0.0);
            if (!step_ok) {
                if (++invalid_run >= 5) { usable = false; break; }
                radius *= 0.5;
                continue;
            }
            invalid_run = 0;
            double cand[7];
#pragma unroll
            for (int j = 0; j < N; ++j) cand[j] = x[j] + delta[j];
            double *C = sums + (cur ^ 1) * 40;
            const bool cok = noc_evaluate(a, b, cand, red, flip, C);
            const double ccost = cok ? C[35] : 1.7976931348623157e308;
            double step_norm = 0.0;
#pragma unroll
            for (int j = 0; j < N; ++j) { const double d = x[j] - cand[j]; step_norm += d * d; }
            step_norm = sqrt(step_norm);
            if (step_norm <= 1e-8 * (x_norm + 1e-8)) { usable = true; break; }
            const double cost_change = cost - ccost;
            if (fabs(cost_change) <= 1e-6 * cost) { usable = true; break; }
            const double rd = cost_change / model_cost_change;
            if (rd > 1e-3) {
                x_norm = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) { x[j] = cand[j]; x_norm += x[j] * x[j]; }
                x_norm = sqrt(x_norm);
                cur ^= 1;
                cost = ccost;
                last_successful = true;
                const double t = 2.0 * rd - 1.0;
                radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
                decrease_factor = 2.0;
            } else {
                radius /= decrease_factor; decrease_factor *= 2.0;
            }
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) a.out_dimpose[(long long)b * 7 + j] = out[j];
        a.out_val[b] = usable ? 1 : 0;
        if (a.out_diag) { a.out_diag[(long long)b * 2] = (double)iteration; a.out_diag[(long long)b * 2 + 1] = cost; }
    }
}
