// pnp_backward_kernel.inc — the backward of `pnp_uncert` (4-DoF, `differentiable=True`): gradients of a loss L(pose, pose_cov)
// with respect to the correspondences, by the implicit function theorem at the refined pose (DESIGN.md §10).
//
// Per object, theta = [yaw, tx, ty, tz] the returned pose, per point i and row k in {u, v}: pi_k(theta, X_i) the projection,
// w = istd, e_k = pi_k - x2d_k, a_k = d pi_k / d theta.  Masks (z clip, per-axis uv clip, inlier mask) are constants.
//   F(theta, x) = sum_{S_LM} w^2 e a = 0 (stationarity of the LM cost), H_F = dF/dtheta = sum_{S_LM} w^2 (a a^T + e da/dtheta)
//   W = -C sym(G) C (C = the returned pose_cov, G = dL/dpose_cov), phi = <W, sum_{S_cov} w^2 a a^T>
//   g = dL/dpose + dphi/dtheta, v = H_F^-1 g, grad_x = dphi/dx - d(v^T F)/dx.
// S_LM = the inlier mask, or every point (lm_all); S_cov = the inlier mask.  One workgroup per object (like exact_hessian_kernel):
// pass 1 reduces H_F (10 values) and dphi/dtheta (4) with block_sum, lane 0 solves the 4x4 system (partial pivoting) and hands v
// over through LDS, pass 2 writes every point's gradients, lanes on consecutive points.  No atomics: the result is deterministic.
// Included by monorun_pnp.hip after hessian_kernel.inc (block_sum, to_f).
//
// Derivatives in closed form.  With q = R(yaw) X + t and the rows N_r = (K q)_r (r = 0, 1, 2; z = N_2), pi_k = N_k / z and for any two
// parameters p, s:  pi_p = (N_kp - pi N_2p) / z,  pi_ps = (N_kps - pi N_2ps - pi_p N_2s - pi_s N_2p) / z.
// The only non-zero second derivatives of q are d2q/dyaw2 = -(R X) rotated (D2 below) and d2q/dyaw dX = dR/dyaw (DE below), so every
// contraction sum_i c_i d a_i / d(.) collapses to a few products (bwd_contract).  For a camera whose third row is (0, 0, 1) H_F is the
// closed form exact_hessian_kernel evaluates (its expressions are the reference's jacobian.py, which assume that row).

struct PnpBwdArgs {
    const void *x2d, *istd, *x3d;
    long long s2[3], sw[3], s3[3];
    const float *K; int K_stride;
    const float *ur, *vr; int r_stride;
    const float *pose;               // (B,4) [yaw,tx,ty,tz]
    const uint8_t *mask;             // (B,P) or null (every point an inlier)
    const uint8_t *valid;            // (B): objects with 0 get zero gradients
    int lm_all;                      // 1: S_LM = every point (inlier_opt_only=False)
    const float *grad_pose;          // (B,4) or null (zero)
    const float *cov, *grad_cov;     // (B,16) each, both or neither
    int B, P; double z_min;
    float *g2, *gw, *g3;             // (B,P,2), (B,P,2), (B,P,3) contiguous, each may be null
    uint8_t *status;                 // (B) or null: 0 gradients written, 1 object not valid, 2 H_F singular or non-finite
};

// One point's geometry: the rows N_r and their derivatives that do not depend on the row k.
struct BwdPoint {
    double z, nu[2];
    double D[3][4];                  // d N_r / d theta
    double D2[3];                    // d2 N_r / d yaw2 (the only non-zero second theta-derivative)
};

// sum_i c_i d a_i / d theta_j for every j, given a (= pi_theta of row k) and pi: (c_0 [j==0] (D2_k - pi D2_2) - (c.a) D_2j - a_j (c.D_2)) / z
__device__ __forceinline__ void bwd_contract_theta(const BwdPoint &q, int k, double pi, const double (&a)[4], const double (&c)[4],
                                                   double iz, double (&out)[4]) {
    const double ca = c[0] * a[0] + c[1] * a[1] + c[2] * a[2] + c[3] * a[3];
    const double cd = c[0] * q.D[2][0] + c[1] * q.D[2][1] + c[2] * q.D[2][2] + c[3] * q.D[2][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (-ca * q.D[2][j] - a[j] * cd) * iz;
    out[0] += c[0] * (q.D2[k] - pi * q.D2[2]) * iz;
}

template <typename T>
__global__ void __launch_bounds__(256) pnp_uncert_backward_kernel(const PnpBwdArgs a) {
    __shared__ double red[2 * 4 * kRedN];
    __shared__ double vsh[5];
    const int b = blockIdx.x, tid = threadIdx.x;
    int flip = 0;
    const bool live = a.valid[b] != 0;
    const bool has_w = a.cov != nullptr;
    const long long ko = (long long)b * a.K_stride, ro = (long long)b * a.r_stride;
    double Kd[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Kd[i] = (double)a.K[ko + i];
    const double lb[2] = { (double)a.ur[ro], (double)a.vr[ro] }, ub[2] = { (double)a.ur[ro + 1], (double)a.vr[ro + 1] };
    const double yaw = (double)a.pose[(long long)b * 4], tx = (double)a.pose[(long long)b * 4 + 1], ty = (double)a.pose[(long long)b * 4 + 2],
                 tz = (double)a.pose[(long long)b * 4 + 3];
    const double sn = sin(yaw), cs = cos(yaw);
    double kr[9], krp[9], kt[3];     // K R, K dR/dyaw, K t
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        kr[3 * r + 0] = Kd[3 * r + 0] * cs - Kd[3 * r + 2] * sn;
        kr[3 * r + 1] = Kd[3 * r + 1];
        kr[3 * r + 2] = Kd[3 * r + 0] * sn + Kd[3 * r + 2] * cs;
        krp[3 * r + 0] = -Kd[3 * r + 0] * sn - Kd[3 * r + 2] * cs;
        krp[3 * r + 1] = 0.0;
        krp[3 * r + 2] = Kd[3 * r + 0] * cs - Kd[3 * r + 2] * sn;
        kt[r] = Kd[3 * r + 0] * tx + Kd[3 * r + 1] * ty + Kd[3 * r + 2] * tz;
    }
    // W = -C sym(G) C (every lane: uniform loads, 128 fp64 FMAs)
    double W[16];
    if (has_w) {
        const float *C = a.cov + (long long)b * 16, *G = a.grad_cov + (long long)b * 16;
        double S[16], CS[16];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) S[4 * i + j] = 0.5 * ((double)G[4 * i + j] + (double)G[4 * j + i]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 4; ++l) s += (double)C[4 * i + l] * S[4 * l + j];
                CS[4 * i + j] = s;
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 4; ++l) s += CS[4 * i + l] * (double)C[4 * l + j];
                W[4 * i + j] = -s;
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)          // phi only sees sym(W); an f32 C need not be exactly symmetric
#pragma unroll
            for (int j = i + 1; j < 4; ++j) { const double s = 0.5 * (W[4 * i + j] + W[4 * j + i]); W[4 * i + j] = s; W[4 * j + i] = s; }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) W[i] = 0.0;
    }
    const T *g2 = (const T *)a.x2d + (long long)b * a.s2[0];
    const T *gw = (const T *)a.istd + (long long)b * a.sw[0];
    const T *g3 = (const T *)a.x3d + (long long)b * a.s3[0];

    // the geometry of point p; false when the point contributes nothing (outside both sets, or z clip)
    auto point = [&](int p, bool &in_lm, bool &in_cov, double (&X)[3], BwdPoint &q) -> bool {
        const bool inl = a.mask ? (a.mask[(long long)b * a.P + p] != 0) : true;
        in_lm = a.lm_all || inl;
        in_cov = inl;
        if (!in_lm && !in_cov) return false;
#pragma unroll
        for (int m = 0; m < 3; ++m) X[m] = (double)to_f(g3[(long long)p * a.s3[1] + m * a.s3[2]]);
        const double Bv = cs * X[0] + sn * X[2], A = -sn * X[0] + cs * X[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double n = kr[3 * r] * X[0] + kr[3 * r + 1] * X[1] + kr[3 * r + 2] * X[2] + kt[r];
            if (r < 2) q.nu[r] = n; else q.z = n;
            q.D[r][0] = Kd[3 * r] * A - Kd[3 * r + 2] * Bv;
            q.D[r][1] = Kd[3 * r]; q.D[r][2] = Kd[3 * r + 1]; q.D[r][3] = Kd[3 * r + 2];
            q.D2[r] = -Kd[3 * r] * Bv - Kd[3 * r + 2] * A;
        }
        return !(q.z < a.z_min);                                         // z clip masks both rows (a NaN depth is kept, as in the Hessian kernel)
    };

    // ---- pass 1: H_F (upper triangle, 10) and dphi/dtheta (4)
    double acc[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) acc[i] = 0.0;
    if (live) {
        for (int p = tid; p < a.P; p += 256) {
            bool in_lm, in_cov;
            double X[3];
            BwdPoint q;
            if (!point(p, in_lm, in_cov, X, q)) continue;
            const double iz = 1.0 / q.z;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double pi = q.nu[k] * iz;
                if (pi < lb[k] || pi > ub[k]) continue;                      // per-axis clip masks this row only
                const double w = (double)to_f(gw[(long long)p * a.sw[1] + k * a.sw[2]]);
                const double e = pi - (double)to_f(g2[(long long)p * a.s2[1] + k * a.s2[2]]);
                double av[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) av[j] = (q.D[k][j] - pi * q.D[2][j]) * iz;
                const double ww = w * w;
                if (in_lm) {
                    // w^2 (a a^T + e da/dtheta); da_i/dtheta_j = ([i==j==0] (D2_k - pi D2_2) - a_i D_2j - a_j D_2i) / z
                    const double we = ww * e * iz;
                    int n = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = i; j < 4; ++j, ++n) {
                            double h = -av[i] * q.D[2][j] - av[j] * q.D[2][i];
                            if (i == 0 && j == 0) h += q.D2[k] - pi * q.D2[2];
                            acc[n] += ww * av[i] * av[j] + we * h;
                        }
                }
                if (in_cov && has_w) {
                    double c[4], d[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[i] = 2.0 * ww * (W[4 * i] * av[0] + W[4 * i + 1] * av[1] + W[4 * i + 2] * av[2] + W[4 * i + 3] * av[3]);
                    bwd_contract_theta(q, k, pi, av, c, iz, d);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[10 + j] += d[j];
                }
            }
        }
    }
    block_sum<4, 14>(acc, red, flip);
    if (tid == 0) {
        bool ok = live;
        double M[4][5];
        {
            int n = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j, ++n) { M[i][j] = acc[n]; M[j][i] = acc[n]; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) M[i][4] = (a.grad_pose ? (double)a.grad_pose[(long long)b * 4 + i] : 0.0) + acc[10 + i];
        // Gauss-Jordan with partial pivoting on the 4x5 tableau, every index static (as in exact_hessian_kernel)
#pragma unroll
        for (int col = 0; col < 4; ++col) {
            if (ok) {
                int piv = col;
                double best = fabs(M[col][col]);
#pragma unroll
                for (int r = col + 1; r < 4; ++r) { const double t = fabs(M[r][col]); if (t > best) { best = t; piv = r; } }
                if (!(best > 0.0)) ok = false;
                else {
#pragma unroll
                    for (int r = col + 1; r < 4; ++r)
                        if (piv == r) {
#pragma unroll
                            for (int j = 0; j < 5; ++j) { const double t = M[col][j]; M[col][j] = M[r][j]; M[r][j] = t; }
                        }
                    const double d = 1.0 / M[col][col];
#pragma unroll
                    for (int j = 0; j < 5; ++j) M[col][j] *= d;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (r != col) {
                            const double f = M[r][col];
#pragma unroll
                            for (int j = 0; j < 5; ++j) M[r][j] -= f * M[col][j];
                        }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ok = ok && isfinite(M[i][4]);
#pragma unroll
        for (int i = 0; i < 4; ++i) vsh[i] = ok ? M[i][4] : 0.0;
        vsh[4] = ok ? 1.0 : 0.0;
        if (a.status) a.status[b] = !live ? 1 : (ok ? 0 : 2);
    }
    __syncthreads();
    const bool ok = vsh[4] != 0.0;
    const double v[4] = { vsh[0], vsh[1], vsh[2], vsh[3] };

    // ---- pass 2: per-point gradients (zeros for points outside both sets, clipped rows and objects without a solution)
    for (int p = tid; p < a.P; p += 256) {
        double gx[2] = { 0.0, 0.0 }, gi[2] = { 0.0, 0.0 }, g3o[3] = { 0.0, 0.0, 0.0 };
        bool in_lm = false, in_cov = false;
        double X[3];
        BwdPoint q;
        if (ok && point(p, in_lm, in_cov, X, q)) {
            const double iz = 1.0 / q.z;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double pi = q.nu[k] * iz;
                if (pi < lb[k] || pi > ub[k]) continue;
                const double w = (double)to_f(gw[(long long)p * a.sw[1] + k * a.sw[2]]);
                const double e = pi - (double)to_f(g2[(long long)p * a.s2[1] + k * a.s2[2]]);
                double av[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) av[j] = (q.D[k][j] - pi * q.D[2][j]) * iz;
                const double ww = w * w;
                const double va = v[0] * av[0] + v[1] * av[1] + v[2] * av[2] + v[3] * av[3];
                double c[4] = { 0.0, 0.0, 0.0, 0.0 };                        // sum_i c_i da_i/dX contracts both terms at once
                double gwk = 0.0;
                if (in_cov && has_w) {
                    double Wa[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) Wa[i] = W[4 * i] * av[0] + W[4 * i + 1] * av[1] + W[4 * i + 2] * av[2] + W[4 * i + 3] * av[3];
                    gwk += 2.0 * w * (av[0] * Wa[0] + av[1] * Wa[1] + av[2] * Wa[2] + av[3] * Wa[3]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[i] += 2.0 * ww * Wa[i];
                }
                double bX[3];                                                // d pi_k / dX
#pragma unroll
                for (int m = 0; m < 3; ++m) bX[m] = (kr[3 * k + m] - pi * kr[6 + m]) * iz;
                if (in_lm) {
                    gx[k] = ww * va;
                    gwk -= 2.0 * w * va * e;
#pragma unroll
                    for (int i = 0; i < 4; ++i) c[i] -= ww * e * v[i];
#pragma unroll
                    for (int m = 0; m < 3; ++m) g3o[m] -= ww * va * bX[m];
                }
                gi[k] = gwk;
                // sum_i c_i da_i/dX_m = (c_0 (KR'_km - pi KR'_2m) - (c.a) KR_2m - b_m (c.D_2)) / z
                const double ca = c[0] * av[0] + c[1] * av[1] + c[2] * av[2] + c[3] * av[3];
                const double cd = c[0] * q.D[2][0] + c[1] * q.D[2][1] + c[2] * q.D[2][2] + c[3] * q.D[2][3];
#pragma unroll
                for (int m = 0; m < 3; ++m) g3o[m] += (c[0] * (krp[3 * k + m] - pi * krp[6 + m]) - ca * kr[6 + m] - bX[m] * cd) * iz;
            }
        }
        const long long o = (long long)b * a.P + p;
        if (a.g2) { a.g2[2 * o] = (float)gx[0]; a.g2[2 * o + 1] = (float)gx[1]; }
        if (a.gw) { a.gw[2 * o] = (float)gi[0]; a.gw[2 * o + 1] = (float)gi[1]; }
        if (a.g3) { a.g3[3 * o] = (float)g3o[0]; a.g3[3 * o + 1] = (float)g3o[1]; a.g3[3 * o + 2] = (float)g3o[2]; }
    }
}
