// epnp_kernel.inc — the reference's own initialiser on the GPU (included by monorun_pnp.hip inside its anonymous namespace):
//     cv2.solvePnPRansac(X, x, K, 0, reprojectionError=thr, iterationsCount=30, flags=SOLVEPNP_EPNP)   and, without a threshold,
//     cv2.solvePnP(X, x, K, 0, flags=SOLVEPNP_EPNP)          (/root/reference/monorun/ops/least_squares/pnp_uncert_cpu.py:33-68)
// for a batch of objects, feeding (init_pose, inlier mask) to the LM launch.  This file: the scalar building blocks (small dense
// linear algebra in registers, beta approximations, Gauss-Newton, absolute orientation, Rodrigues, the istd candidate stage, the
// RANSAC bookkeeping); epnp_eig_low4.inc: the 12x12 eigen-solver; epnp_stages.inc: the launches.
//
// OpenCV is third-party and absent; the arithmetic followed here is the published algorithm as the test infrastructure specifies
// it operation for operation (EPnP: control points by PCA, barycentric coordinates, M^T M, its four smallest eigenvectors, three
// beta approximations x 5 Gauss-Newton steps, absolute orientation, best of three; RANSAC: cv::RNG((uint64)-1), 5-point subsets
// with rejection of repeats, float32 squared reprojection error <= thr^2, acceptance above max(best, 4), RANSACUpdateNumIters,
// re-fit on the inliers).  Mapping onto the machine:
//   * the RNG's subset indices do not depend on any model, so all 30 minimal sets are known up front and the 30 EPnP
//     hypotheses of every object are solved SPECULATIVELY and in parallel; their consensus counts are taken by a workgroup per
//     object, and the RANSAC loop — acceptance, adaptive iteration count — is then replayed over the counts in RNG order, so the
//     result is the sequential algorithm's;
//   * sums over the points of the re-fit are 64 interleaved partials per wave + the wave's permlane/DPP butterfly;
//   * no fused multiply-add except where written, IEEE division and square root: hypotheses, masks and the initial pose can be
//     compared bit for bit with the CPU restatement (only acos / sin / cos / log / pow come from the device math library).
#define MR_EXACT _Pragma("clang fp contract(off)")

constexpr int kEpMaxIters = 30;      // iterationsCount of the reference's call (pnp_uncert_cpu.py:38)

// ---------------------------------------------------------------------------- small dense linear algebra in registers
// cyclic Jacobi eigen-decomposition of a symmetric 3x3 (the PCA of the control points): eigenvalues descending, eigenvectors
// in the ROWS of vt
// the Jacobi rotation of [[a, g], [g, b]] from dl = b - a, g2 = 2 g: two square roots and ONE division (oracle/epnp.inc epnp_jacobi_cs)
__device__ __forceinline__ void ep_jacobi_cs(const double dl, const double g2, double &c, double &s) {
    MR_EXACT
    const double h = sqrt(fma(dl, dl, g2 * g2));
    const double den = fabs(dl) + h, num = dl >= 0.0 ? g2 : -g2;
    const double ir = 1.0 / sqrt(fma(den, den, num * num));
    c = den * ir; s = num * ir;
}
__device__ __forceinline__ void ep_eig3(const double (&Ain)[9], double (&w)[3], double (&vt)[9]) {
    MR_EXACT
    double A[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { A[i] = Ain[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dia += A[3 * i + i] * A[3 * i + i];
#pragma unroll
            for (int j = i + 1; j < 3; ++j) off += A[3 * i + j] * A[3 * i + j];
        }
        if (off <= 1e-32 * dia || off == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[3 * p + q];
                if (apq != 0.0) {
                    double c, s;
                    ep_jacobi_cs(A[3 * q + q] - A[3 * p + p], apq + apq, c, s);
#pragma unroll
                    for (int k = 0; k < 3; ++k) { const double akp = A[3 * k + p], akq = A[3 * k + q]; A[3 * k + p] = fma(c, akp, -(s * akq)); A[3 * k + q] = fma(s, akp, c * akq); }
#pragma unroll
                    for (int k = 0; k < 3; ++k) { const double apk = A[3 * p + k], aqk = A[3 * q + k]; A[3 * p + k] = fma(c, apk, -(s * aqk)); A[3 * q + k] = fma(s, apk, c * aqk); }
#pragma unroll
                    for (int k = 0; k < 3; ++k) { const double vkp = V[3 * k + p], vkq = V[3 * k + q]; V[3 * k + p] = fma(c, vkp, -(s * vkq)); V[3 * k + q] = fma(s, vkp, c * vkq); }
                }
            }
    }
    // exchange sort of (value, column) pairs, descending, the specification's comparison sequence
    double val[3] = { A[0], A[4], A[8] };
    int ord[3] = { 0, 1, 2 };
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j)
            if (val[j] > val[i]) { const double tv = val[i]; val[i] = val[j]; val[j] = tv; const int to = ord[i]; ord[i] = ord[j]; ord[j] = to; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        w[i] = val[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) vt[3 * i + k] = ord[i] == 0 ? V[3 * k] : (ord[i] == 1 ? V[3 * k + 1] : V[3 * k + 2]);
    }
}

// one-sided (Hestenes) Jacobi SVD of an M x N matrix (row-major), M >= N: A = U diag(w) V^T, w descending; u is M x N, v is N x N
template <int M, int N>
__device__ __forceinline__ void ep_svd(const double (&Ain)[M * N], double (&w)[N], double (&u)[M * N], double (&v)[N * N]) {
    MR_EXACT
    double A[M * N], V[N * N];
#pragma unroll
    for (int i = 0; i < M * N; ++i) A[i] = Ain[i];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[N * i + j] = (i == j) ? 1.0 : 0.0;
    if constexpr (M == 6) {
        // the 6-row systems of the beta approximations: columns by descending norm before the first sweep (oracle/epnp.inc epnp_svd:
        // 4.4 instead of 5.6 sweeps on config-2 data); V starts as that permutation.  Exchange sort, every index static.
        double nr[N];
        int od[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) t = fma(A[N * k + j], A[N * k + j], t);
            nr[j] = t; od[j] = j;
        }
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = i + 1; j < N; ++j) {
                const bool sw = nr[j] > nr[i];
                const double tn = nr[i]; nr[i] = sw ? nr[j] : nr[i]; nr[j] = sw ? tn : nr[j];
                const int to = od[i]; od[i] = sw ? od[j] : od[i]; od[j] = sw ? to : od[j];
#pragma unroll
                for (int k = 0; k < M; ++k) { const double t = A[N * k + i]; A[N * k + i] = sw ? A[N * k + j] : t; A[N * k + j] = sw ? t : A[N * k + j]; }
            }
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) V[N * k + j] = (od[j] == k) ? 1.0 : 0.0;
    }
    // one pair visit in three pieces, so that two visits that share no column can be laid side by side and so that the rotation's (c, s)
    // — two square roots and a division, ~40 dependent instructions — is only computed when some lane of the WAVE rotates a pair of the
    // round: the last sweep of every decomposition rotates nothing, and the late sweeps little (the values are what they were: a lane
    // that does not rotate never used its (c, s))
    auto dots = [&](const int p, const int q, double &dl, double &g2) -> bool {
        double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) { a = fma(A[N * k + p], A[N * k + p], a); b = fma(A[N * k + q], A[N * k + q], b); g = fma(A[N * k + p], A[N * k + q], g); }
        dl = b - a; g2 = g + g;
        return !(g == 0.0 || g * g <= (4.0 * 2.220446049250313e-16 * 2.220446049250313e-16) * (a * b));
    };
    auto rotate = [&](const int p, const int q, const double c, const double s_) {
#pragma unroll
        for (int k = 0; k < M; ++k) { const double x = A[N * k + p], y = A[N * k + q]; A[N * k + p] = fma(c, x, -(s_ * y)); A[N * k + q] = fma(s_, x, c * y); }
#pragma unroll
        for (int k = 0; k < N; ++k) { const double x = V[N * k + p], y = V[N * k + q]; V[N * k + p] = fma(c, x, -(s_ * y)); V[N * k + q] = fma(s_, x, c * y); }
    };
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        if constexpr (N == 5) {
            // the specification's pair order: a round-robin tournament, two column-disjoint pairs per round — their (c, s) chains run interleaved
            constexpr int R[5][4] = { { 0, 1, 2, 3 }, { 0, 2, 1, 4 }, { 0, 3, 2, 4 }, { 0, 4, 1, 3 }, { 1, 2, 3, 4 } };
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                double dl0, g20, dl1, g21;
                const bool go0 = dots(R[r][0], R[r][1], dl0, g20);
                const bool go1 = dots(R[r][2], R[r][3], dl1, g21);
                if (__builtin_amdgcn_ballot_w64(go0 || go1) != 0ull) {
                    double c0, s0, c1, s1;
                    ep_jacobi_cs(dl0, g20, c0, s0);
                    ep_jacobi_cs(dl1, g21, c1, s1);
                    if (go0) { rotated = true; rotate(R[r][0], R[r][1], c0, s0); }
                    if (go1) { rotated = true; rotate(R[r][2], R[r][3], c1, s1); }
                }
            }
        } else {
            static_assert(N <= 3, "the tournament order restricted to N columns is the lexicographic one only for N <= 3");
#pragma unroll
            for (int p = 0; p < N - 1; ++p)
#pragma unroll
                for (int q = p + 1; q < N; ++q) {
                    double dl, g2;
                    const bool go = dots(p, q, dl, g2);
                    if (__builtin_amdgcn_ballot_w64(go) != 0ull) {
                        double c, s_;
                        ep_jacobi_cs(dl, g2, c, s_);
                        if (go) { rotated = true; rotate(p, q, c, s_); }
                    }
                }
        }
        if (!rotated) break;
    }
    double nrm[N], val[N];
    int ord[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) s += A[N * k + j] * A[N * k + j];
        nrm[j] = sqrt(s); val[j] = nrm[j]; ord[j] = j;
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i + 1; j < N; ++j)
            if (val[j] > val[i]) { const double tv = val[i]; val[i] = val[j]; val[j] = tv; const int to = ord[i]; ord[i] = ord[j]; ord[j] = to; }
#pragma unroll
    for (int j = 0; j < N; ++j) {
        w[j] = val[j];
        const double rn = 1.0 / val[j];                       // one division per column
#pragma unroll
        for (int k = 0; k < M; ++k) {
            double a = A[N * k];
#pragma unroll
            for (int c = 1; c < N; ++c) a = (ord[j] == c) ? A[N * k + c] : a;
            u[N * k + j] = val[j] > 0.0 ? a * rn : 0.0;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double a = V[N * k];
#pragma unroll
            for (int c = 1; c < N; ++c) a = (ord[j] == c) ? V[N * k + c] : a;
            v[N * k + j] = a;
        }
    }
}

// x = pinv(A) b through the SVD (singular values <= 2 eps sum(w) count as zero)
template <int M, int N>
__device__ __forceinline__ void ep_svd_solve(const double (&A)[M * N], const double (&b)[M], double (&x)[N]) {
    MR_EXACT
    double w[N], u[M * N], v[N * N], thr = 0.0;
    ep_svd<M, N>(A, w, u, v);
#pragma unroll
    for (int j = 0; j < N; ++j) thr += w[j];
    thr *= 2.0 * 2.220446049250313e-16;
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (w[j] > thr) {
            double ub = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) ub += u[N * k + j] * b[k];
            ub /= w[j];
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] += v[N * i + j] * ub;
        }
    }
}

// Householder QR least squares of the Gauss-Newton step (6 x 4); false on a zero column (step skipped)
__device__ __forceinline__ bool ep_qr_solve(double (&A)[24], double (&b)[6], double (&X)[4]) {
    MR_EXACT
    constexpr int nr = 6, nc = 4;
    double A1[4], A2[4], rA1[4], rA2[4];              // one reciprocal per pivot quantity, taken when it is formed (oracle/epnp.inc epnp_qr_solve)
    bool ok = true;
#pragma unroll
    for (int k = 0; k < nc; ++k) {
        if (ok) {
            double eta = fabs(A[nc * k + k]);
#pragma unroll
            for (int i = k + 1; i < nr; ++i) { const double e = fabs(A[nc * (i - 1) + k]); if (eta < e) eta = e; }
            if (eta == 0.0) ok = false;
            else {
                const double inv_eta = 1.0 / eta;
                double sum2 = 0.0;
#pragma unroll
                for (int i = k; i < nr; ++i) { A[nc * i + k] *= inv_eta; sum2 += A[nc * i + k] * A[nc * i + k]; }
                double sigma = sqrt(sum2);
                if (A[nc * k + k] < 0) sigma = -sigma;
                A[nc * k + k] += sigma;
                A1[k] = sigma * A[nc * k + k];
                A2[k] = -eta * sigma;
                rA1[k] = 1.0 / A1[k]; rA2[k] = 1.0 / A2[k];
#pragma unroll
                for (int j = k + 1; j < nc; ++j) {
                    double sum = 0.0;
#pragma unroll
                    for (int i = k; i < nr; ++i) sum += A[nc * i + k] * A[nc * i + j];
                    const double tau = sum * rA1[k];
#pragma unroll
                    for (int i = k; i < nr; ++i) A[nc * i + j] -= tau * A[nc * i + k];
                }
            }
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < nc; ++j) {
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < nr; ++i) tau += A[nc * i + j] * b[i];
        tau *= rA1[j];
#pragma unroll
        for (int i = j; i < nr; ++i) b[i] -= tau * A[nc * i + j];
    }
    X[nc - 1] = b[nc - 1] * rA2[nc - 1];
#pragma unroll
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0.0;
#pragma unroll
        for (int j = i + 1; j < nc; ++j) sum += A[nc * i + j] * X[j];
        X[i] = (b[i] - sum) * rA2[i];
    }
    return true;
}

__device__ __forceinline__ double ep_dot3(const double *a, const double *b) { MR_EXACT return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ double ep_dist2(const double *a, const double *b) {
    MR_EXACT
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// one row of the Gauss-Newton system: Jacobian row A[0..3] and residual b of distance constraint i (L row r, rho_i) at the current betas
__device__ __forceinline__ void ep_gn_row(const double (&r)[10], const double rho_i, const double (&betas)[4], double *A, double &b) {
    MR_EXACT
    A[0] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3];
    A[1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3];
    A[2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3];
    A[3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3];
    b = rho_i - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                 r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                 r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3]);
}

// The three beta approximations (N = 1, 2, 3: [B11 B12 B13 B14], [B11 B12 B22], [B11 B12 B22 B13 B23] from L (6x10) and rho) with the
// candidate as a per-LANE value (cand = N - 1): the three least-squares systems are embedded
// in ONE 6 x 5 system whose unused columns are zero — [L0 L1 L3 L6 0], [L0 L1 L2 0 0], [L0 L1 L2 L3 L4].  A zero column never
// rotates in the one-sided Jacobi SVD (its inner products are exact zeros), sorts behind every column that has a norm, contributes an
// exact +0 to the threshold sum and is skipped by the pseudo-inverse: every operation on the live columns is the operation of the
// 6 x 4 / 6 x 3 / 6 x 5 solve of the specification (oracle/epnp.inc epnp_solve), in the same order — bit-identical results, one code path for the lanes of a wave.
__device__ __forceinline__ void ep_betas_from_x5(const double (&x5)[5], const int cand, double (&be)[4]) {
    MR_EXACT
    if (cand == 0) {
        if (x5[0] < 0) { be[0] = sqrt(-x5[0]); be[1] = -x5[1] / be[0]; be[2] = -x5[2] / be[0]; be[3] = -x5[3] / be[0]; }
        else           { be[0] = sqrt(x5[0]);  be[1] = x5[1] / be[0];  be[2] = x5[2] / be[0];  be[3] = x5[3] / be[0]; }
    } else {
        if (x5[0] < 0) { be[0] = sqrt(-x5[0]); be[1] = (x5[2] < 0) ? sqrt(-x5[2]) : 0.0; }
        else           { be[0] = sqrt(x5[0]);  be[1] = (x5[2] > 0) ? sqrt(x5[2]) : 0.0; }
        if (x5[1] < 0) be[0] = -be[0];
        be[2] = cand == 2 ? x5[3] / be[0] : 0.0; be[3] = 0.0;
    }
}

// R = U V^T from the SVD of the 3x3 correlation, reflection fixed by the determinant; t = pc0 - R pw0
__device__ __forceinline__ void ep_abt_to_pose(const double (&abt)[9], const double (&pc0)[3], const double (&pw0)[3], double (&R)[9], double (&t)[3]) {
    MR_EXACT
    double d[3], U[9], V[9];
    ep_svd<3, 3>(abt, d, U, V);
    if (!(d[2] > 0.0)) {
        U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = pc0[j] - ep_dot3(&R[3 * j], pw0);
}

// rotation matrix -> rotation vector (cv::Rodrigues on a 3x3: re-orthogonalise with the SVD, then the closed form)
__device__ __forceinline__ void ep_rodrigues_to_vec(const double (&Rin)[9], double (&r)[3]) {
    MR_EXACT
    double w[3], U[9], V[9], R[9];
    ep_svd<3, 3>(Rin, w, U, V);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    double theta = acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0.0; return; }
        double t = (R[0] + 1) * 0.5; rx = sqrt(t > 0.0 ? t : 0.0);
        t = (R[4] + 1) * 0.5; ry = sqrt(t > 0.0 ? t : 0.0) * (R[1] < 0 ? -1.0 : 1.0);
        t = (R[8] + 1) * 0.5; rz = sqrt(t > 0.0 ? t : 0.0) * (R[2] < 0 ? -1.0 : 1.0);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && ((R[5] > 0) != (ry * rz > 0))) rz = -rz;
        theta /= sqrt(rx * rx + ry * ry + rz * rz);
        r[0] = rx * theta; r[1] = ry * theta; r[2] = rz * theta;
    } else {
        const double vth = theta / (2.0 * s);
        r[0] = rx * vth; r[1] = ry * vth; r[2] = rz * vth;
    }
}
__device__ __forceinline__ void ep_rodrigues_to_mat(const double (&r)[3], double (&R)[9]) {
    MR_EXACT
    const double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < 2.220446049250313e-16) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
    const double x = r[0] * it, y = r[1] * it, z = r[2] * it;
    R[0] = c + c1 * x * x; R[1] = c1 * x * y - s * z; R[2] = c1 * x * z + s * y;
    R[3] = c1 * x * y + s * z; R[4] = c + c1 * y * y; R[5] = c1 * y * z - s * x;
    R[6] = c1 * x * z - s * y; R[7] = c1 * y * z + s * x; R[8] = c + c1 * z * z;
}

// ---------------------------------------------------------------------------- sample-level pieces
using EpCam = K4;       // { fx, fy, cx, cy } in doubles (pnp_kernel.inc)

__device__ __forceinline__ double ep_psum5(double t0, double t1, double t2, double t3, double t4) {
    MR_EXACT
    return ((t0 + t1) + (t2 + t3)) + t4;             // the 64-partial butterfly (strides 32, 16, 1, 2, 4, 8) on five occupied partials
}

// (own text, like stage 1 of pnp_uncert_kernel: with the sums and the list loop as shared functions the code of epnp_front_kernel moves — HISTORY.md, round 12)
// stage 1 of the per-object kernels: istd inlier mask with numpy's float32 summation order (pnp_uncert_cpu.py:164-168) and the
// ascending candidate list.  Three barriers in all: after the sums, after the ballots, after the list (the last one is the
// caller's).  Returns the number of candidates = entries of slist.  pl_*: the summation-plan entries this lane prefetched.
template <int WPO, typename T, typename ARGS>
__device__ __forceinline__ int istd_mask_stage(const ARGS &a, const Tile<T> &tl, const int P, const int nchunk, const int npt, const int tid, const int lane,
                                               const int wid, float *sres, float *snode, unsigned long long *sball, uint8_t *smask, uint16_t *slist,
                                               const int pl_off, const int pl_len, const int pl_l, const int pl_r, const unsigned pl_ls0, const unsigned pl_ls1) {
    constexpr int NT = 64 * WPO;
    int n = 0;                                          // number of candidates = entries of slist
    if (a.flags & MR_NO_ISTD_MASK) {
        for (int p = tid; p < P; p += NT) { smask[p] = 1; slist[p] = (uint16_t)p; }
        n = P;
    } else {
        if (a.mean_mode == MR_MEAN_SEQUENTIAL) {
            // numpy reduces a C-contiguous (B,P,2) float32 array over axis 1 strictly in p order
            if (tid < 2) {
                float s = 0.0f;
                if (tid == 0) { for (int p = 0; p < P; ++p) s += tl.wu(p); }
                else          { for (int p = 0; p < P; ++p) s += tl.wv(p); }
                sres[tid] = s;
            }
        } else {
            // numpy pairwise summation (point axis contiguous): 8 strided accumulators per <=128 block, their fixed
            // ((0+1)+(2+3))+((4+5)+(6+7)) combination, the block's tail, then the combine tree.  Each channel is summed
            // entirely inside ONE wave (lane = leaf*8 + accumulator; xor-butterflies give the same additions in the same
            // order; the tree runs wave-synchronously through LDS), so no workgroup barrier is spent on it.
            const int nl = a.plan.n_leaves;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (wid != (c % WPO)) continue;
                float *nd = snode + c * 2 * a.nla;
                for (int l0 = 0; l0 < nl; l0 += 8) {
                    const int leaf = l0 + (lane >> 3), j = lane & 7;
                    const bool act = leaf < nl;
                    const int off = (l0 == 0) ? pl_off : (act ? (int)a.plan.leaf_off[leaf] : 0);
                    const int len = (l0 == 0) ? pl_len : (act ? (int)a.plan.leaf_len[leaf] : 0);
                    float acc = 0.0f;
                    if (len < 8) {
                        if (j == 0) for (int i = 0; i < len; ++i) acc += c ? tl.wv(off + i) : tl.wu(off + i);
                    } else {
                        const int n8 = len >> 3;                   // <= 16 strided terms
                        float vv[16];
#pragma unroll
                        for (int i = 0; i < 16; ++i) { const int q = off + ((i < n8) ? i : 0) * 8 + j; vv[i] = c ? tl.wv(q) : tl.wu(q); }
                        acc = vv[0];
#pragma unroll
                        for (int i = 1; i < 16; ++i) acc = (i < n8) ? acc + vv[i] : acc;
                    }
                    float r = acc;
                    r = r + dpp_f<0xB1>(r);                        // (0+1) (2+3) (4+5) (6+7)
                    r = r + dpp_f<0x4E>(r);                        // ((0+1)+(2+3)) ((4+5)+(6+7))
                    r = r + dpp_f<0x141>(r);                       // the two quads of the 8-lane group (row_half_mirror)
                    float res = (len < 8) ? acc : r;
                    if (j == 0 && len >= 8) for (int i = len - (len & 7); i < len; ++i) res += c ? tl.wv(off + i) : tl.wu(off + i);
                    if (act && j == 0) nd[leaf] = res;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                // internal node k (< 64) is evaluated by lane k at its level; level boundaries = bytes of the prefetched words
                auto level_start = [&](int lv) { return lv < 8 ? (int)(((lv < 4 ? pl_ls0 : pl_ls1) >> (8 * (lv & 3))) & 0xffu) : (int)a.plan.level_start[lv]; };
                for (int lv = 0; lv < a.plan.n_levels; ++lv) {
                    const int n0 = level_start(lv), n1 = level_start(lv + 1);
                    if (lane >= n0 && lane < n1) nd[nl + lane] = nd[pl_l] + nd[pl_r];
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                }
                if (lane == 0) sres[c] = nd[a.plan.root];
            }
        }
        __syncthreads();
        // mean = sum / P ; threshold = float32(thres) * mean ; both axes must pass (pnp_uncert_cpu.py:164-168)
        const float thr_u = a.istd_thres * (sres[0] / (float)P);
        const float thr_v = a.istd_thres * (sres[1] / (float)P);
        for (int i = 0; i < npt; ++i) {
            const int p = i * NT + tid;                            // chunk p >> 6 = i * WPO + wid is wave-uniform
            const bool in = (p < P) && tl.weights_pass(p < P ? p : 0, thr_u, thr_v);
            if (p < P) smask[p] = in ? 1 : 0;
            const unsigned long long bal = __ballot(in);
            if (lane == 0 && i * WPO + wid < nchunk) sball[i * WPO + wid] = bal;
        }
        __syncthreads();
        int ex0, ex1;
        n = scan_chunks(sball, nchunk, lane, ex0, ex1);
        if (!(n > 4)) {                                            // pnp_uncert_cpu.py:23-32: too few -> every point
            for (int p = tid; p < P; p += NT) { smask[p] = 1; slist[p] = (uint16_t)p; }
            n = P;
        } else {
            for (int i = 0; i < npt; ++i) {
                const int chunk = i * WPO + wid;
                if (chunk >= nchunk) break;
                const unsigned long long bal = sball[chunk];
                const int base = chunk_base(chunk, ex0, ex1);
                if ((bal >> lane) & 1ull) slist[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)(chunk * 64 + lane);
            }
        }
    }
    return n;
}


// RANSACUpdateNumIters(p, ep, modelPoints, maxIters) of ptsetreg.cpp
__device__ __forceinline__ int ep_update_iters(double p, double ep, int model_points, int max_iters) {
    MR_EXACT
    p = p < 0.0 ? 0.0 : (p > 1.0 ? 1.0 : p);
    ep = ep < 0.0 ? 0.0 : (ep > 1.0 ? 1.0 : ep);
    double num = 1.0 - p; if (num < 2.2250738585072014e-308) num = 2.2250738585072014e-308;
    double denom = 1.0 - pow(1.0 - ep, (double)model_points);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num); denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)lrint(num / denom);
}

// is candidate (X, img) an inlier of the model (R, t)?  PnPRansacCallback::computeError: projectPoints in double, the projected
// point stored as float32, difference and squared norm in float32
__device__ __forceinline__ bool ep_is_inlier(const EpCam &k, const double (&R)[9], const double (&t)[3], float X_, float Y_, float Z_, float u, float v, float thr2) {
    MR_EXACT
    const double X = X_, Y = Y_, Z = Z_;
    const double x = R[0] * X + R[1] * Y + R[2] * Z + t[0], y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
    double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
    z = z ? 1.0 / z : 1.0;
    const float pu = (float)(x * z * k.fx + k.cx), pv = (float)(y * z * k.fy + k.cy);
    const float du = u - pu, dv = v - pv;
    const float err = du * du + dv * dv;
    return err <= thr2;
}

constexpr int kEpThreads = 256;
