// kitti_eval_kernel.inc — N2 (SURVEY.md §8f): the KITTI object evaluator's device side.
//
// Reference: monorun/core/evaluation/kitti_utils/eval.py (numba-jitted CPU loops) and rotate_iou.py (numba-CUDA
// rotated IoU).  numba does not exist here and numba-CUDA cannot run on ROCm; the evaluator's three loop nests become
// three embarrassingly parallel HIP kernels over flat, offset-indexed arrays (HBM-bound integer/compare work):
//   kitti_overlap_kernel   one thread per (detection, label) pair of the SAME image  (eval.py:84-158, rotate_iou.py:256-281)
//                          — the reference computes whole cross-image "part" matrices and slices the diagonal blocks out
//                          (eval.py:341-416); only the diagonal blocks are computed here.  On identical boxes the rotated
//                          overlap is 1, a deliberate departure from the numba kernel's value there (1/3 or 0 of the area):
//                          edge_inside_area_t below
//   kitti_match_kernel     one thread per (class x difficulty x overlap "combo", [threshold,] image): the sequential greedy
//                          assignment compute_statistics_jit (eval.py:161-279)
//   kitti_reduce_kernel    one thread per (combo, threshold): ordered sum over images (fused_compute_statistics, eval.py:291-338)
// Box rows (double[12]): x1 y1 x2 y2 | x y z | l h w | ry | score.

constexpr int kEvalMaxDet = 512;          // detections per image the matching kernel supports
constexpr int kEvalSamples = 41;          // N_SAMPLE_PTS, eval.py:481

__device__ __forceinline__ float t_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double t_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float t_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double t_min(double a, double b) { return fmin(a, b); }
// torch's / numpy's element-wise forms, which keep a NaN where fminf / fmaxf drop it (the 3-D IoU, the projection loss, the score head)
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }       // torch.min / np.minimum: NaN from either side
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }       // np.maximum
__device__ __forceinline__ float clamp_lo(float x, float lo) { return x < lo ? lo : x; }               // clamp(min=lo); torch.relu is clamp_lo(x, 0): NaN stays
__device__ __forceinline__ float clamp_hi(float x, float hi) { return x > hi ? hi : x; }               // clamp(max=hi), NaN stays

// a*b + c*d rounded operation by operation, never fused into an FMA
template <typename T>
__device__ __forceinline__ T dot2_unfused(T a, T b, T c, T d) {
#pragma clang fp contract(off)
    return a * b + c * d;
}
// z of (ux, uy) x (vx, vy), likewise
template <typename T>
__device__ __forceinline__ T cross2_unfused(T ux, T uy, T vx, T vy) { return dot2_unfused(ux, vy, -uy, vx); }

__device__ __forceinline__ float t_abs(float a) { return fabsf(a); }
__device__ __forceinline__ double t_abs(double a) { return fabs(a); }
template <typename T> struct CollinearTol;      // 64 ulp: the corners carry a few ulp of their box's size each, the cross products some more
template <> struct CollinearTol<float> { static constexpr float value = 64.0f * 1.1920929e-07f; };
template <> struct CollinearTol<double> { static constexpr double value = 64.0 * 2.220446049250313e-16; };

// Whether segment p -> r and edge a -> b lie on one line: each one's two ends within tol of the other's line.  f0 is p against the
// edge's line.  The four cross products are the same numbers when segment and edge change places.
template <typename T>
__device__ __forceinline__ bool on_one_line(T px, T py, T rx, T ry, T ax, T ay, T bx, T by, T f0, T tol) {
    const T ex = bx - ax, ey = by - ay, dx = rx - px, dy = ry - py;
    const T f1 = cross2_unfused(ex, ey, rx - ax, ry - ay);                                                       // r against the edge's line
    const T g0 = cross2_unfused(dx, dy, ax - px, ay - py), g1 = cross2_unfused(dx, dy, bx - px, by - py);        // a, b against the segment's
    return t_max(t_max(t_abs(f0), t_abs(f1)), t_max(t_abs(g0), t_abs(g1))) <= tol;
}

// length-weighted boundary integral of the part of segment p -> r that lies inside the convex CCW polygon q (Cyrus-Beck parametric
// clipping, no dynamic arrays).  Any scalar type (float: the NMS, double: the evaluator and the 3-D IoU).  The intersection's
// boundary is the first rectangle's segments inside the second (CLOSED) plus the second's inside the first (not CLOSED), so a stretch
// of boundary that both rectangles have must come from exactly one of the two calls that meet it.  One rule decides that, for a
// segment and an edge of q that lie on one line:
//   - CLOSED, and the segment runs the way the edge runs (the interiors are on the same side: identical boxes, a box inside the other
//     on a common edge): the edge does not clip the segment, so it counts;
//   - CLOSED, and it runs the other way (the interiors are on opposite sides: boxes that only touch): it does not count;
//   - not CLOSED: it does not count.
// So coincident edges of the same direction are counted once and those of opposite direction never.  "On one line" means that each
// one's two ends are within CollinearTol of the other's line: the four cross products against the product of the two L1 lengths.
// The test reads the same four numbers whichever of the two is the segment, so both calls decide alike, also for edges that coincide
// only to the rounding of their corners (turned boxes with a common centre line), where the signs of f0 and den are noise.
// Every product here is rounded operation by operation: as FMAs, den of an edge against itself is the rounding residue of a product
// instead of 0, and the result would rest on what the compiler contracts.
template <typename T, bool CLOSED>
__device__ __forceinline__ T edge_inside_area_t(T px, T py, T rx, T ry, const T (&qx)[4], const T (&qy)[4]) {
    const T dx = rx - px, dy = ry - py;
    T t0 = T(0), t1 = T(1);
    bool empty = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const T ax = qx[e], ay = qy[e], bx = qx[(e + 1) & 3], by = qy[(e + 1) & 3];
        const T ex = bx - ax, ey = by - ay;                         // (-ey, ex) is the inward normal of a CCW edge
        const T f0 = cross2_unfused(ex, ey, px - ax, py - ay), den = cross2_unfused(ex, ey, dx, dy);          // p against the edge's line
        const T tol = CollinearTol<T>::value * ((t_abs(ex) + t_abs(ey)) * (t_abs(dx) + t_abs(dy)));
        // den is f1 - f0 but for rounding, far below tol: only a nearly parallel pair can be on one line (|den| is the same in both calls)
        if (t_abs(den) <= T(3) * tol && tol > T(0) && on_one_line(px, py, rx, ry, ax, ay, bx, by, f0, tol)) {
            if (!CLOSED || dot2_unfused(dx, ex, dy, ey) < T(0)) empty = true;
        }
        else if (den > T(0)) t0 = t_max(t0, -f0 / den);
        else if (den < T(0)) t1 = t_min(t1, -f0 / den);
        else if (CLOSED ? (f0 < T(0)) : (f0 <= T(0))) empty = true;
    }
    if (empty || !(t1 > t0)) return T(0);
    const T x0 = px + t0 * dx, y0 = py + t0 * dy, x1 = px + t1 * dx, y1 = py + t1 * dy;
    return T(0.5) * (x0 * y1 - x1 * y0);
}

// corners of [cx, cy, dx, dy, angle] with the evaluator's convention (rotate_iou.py:204-227), returned counter-clockwise
// and relative to (ox, oy)
__device__ __forceinline__ void eval_corners(const double (&b)[5], double ox, double oy, double (&px)[4], double (&py)[4]) {
    const double c = cos(b[4]), s = sin(b[4]);
    const double hx = 0.5 * b[2], hy = 0.5 * b[3];
    const double lx[4] = { -hx, hx, hx, -hx }, ly[4] = { -hy, -hy, hy, hy };      // CCW when hx*hy > 0
#pragma unroll
    for (int k = 0; k < 4; ++k) { px[k] = c * lx[k] + s * ly[k] + (b[0] - ox); py[k] = -s * lx[k] + c * ly[k] + (b[1] - oy); }
    if (hx * hy < 0.0) { const double tx = px[1], ty = py[1]; px[1] = px[3]; py[1] = py[3]; px[3] = tx; py[3] = ty; }
}

__device__ __forceinline__ double eval_rotated_intersection(const double (&a)[5], const double (&b)[5]) {
    double ax[4], ay[4], bx[4], by[4];
    eval_corners(a, a[0], a[1], ax, ay);
    eval_corners(b, a[0], a[1], bx, by);
    double ov = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ov += edge_inside_area_t<double, true>(ax[i], ay[i], ax[(i + 1) & 3], ay[(i + 1) & 3], bx, by);
        ov += edge_inside_area_t<double, false>(bx[i], by[i], bx[(i + 1) & 3], by[(i + 1) & 3], ax, ay);
    }
    return fmax(ov, 0.0);
}

// image_box_overlap (eval.py:84-112) in arithmetic type T, operation for operation (no contraction)
template <typename T>
__device__ __forceinline__ T eval_image_overlap(const T b0, const T b1, const T b2, const T b3, const T q0, const T q1, const T q2, const T q3, int criterion) {
#pragma clang fp contract(off)
    const T qa = (q2 - q0) * (q3 - q1);
    const T iw = t_min(b2, q2) - t_max(b0, q0);
    if (!(iw > T(0))) return T(0);
    const T ih = t_min(b3, q3) - t_max(b1, q1);
    if (!(ih > T(0))) return T(0);
    const T ba = (b2 - b0) * (b3 - b1);
    T ua;
    if (criterion == -1) ua = ba + qa - iw * ih;
    else if (criterion == 0) ua = ba;
    else if (criterion == 1) ua = qa;
    else ua = T(1);
    return iw * ih / ua;
}

template <typename T>
__device__ __forceinline__ double eval_d3(const double *d, const double *g, float rinc) {
#pragma clang fp contract(off)
    // d3_box_overlap_kernel (eval.py:121-150), criterion -1; y is the bottom of the box, pointing down
    if (!(rinc > 0.0f)) return (double)rinc;                   // untouched entries keep the (non-positive) BEV value
    const T yb = (T)d[5], hb = (T)d[8], yq = (T)g[5], hq = (T)g[8];
    const T iw = t_min(yb, yq) - t_max(yb - hb, yq - hq);
    if (!(iw > T(0))) return 0.0;
    const T a1 = (T)d[7] * hb * (T)d[9], a2 = (T)g[7] * hq * (T)g[9];
    const T inc = iw * (T)rinc;
    const T ua = a1 + a2 - inc;
    return (double)(float)(inc / ua);
}

__device__ __forceinline__ int eval_find_image(const long long *off, int n, long long p) {
    int lo = 0, hi = n;                                        // largest i with off[i] <= p
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(256) kitti_overlap_kernel(int metric, int arith32, int out32, int n_img, const long long *dt_off,
                                                            const long long *gt_off, const long long *ov_off, const double *dt_box,
                                                            const double *gt_box, double *ov) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= ov_off[n_img]) return;
    const int img = eval_find_image(ov_off, n_img, p);
    const long long ng = gt_off[img + 1] - gt_off[img];
    const long long r = p - ov_off[img];
    const double *d = dt_box + (dt_off[img] + r / ng) * 12, *g = gt_box + (gt_off[img] + r % ng) * 12;
    double res;
    if (metric == 0) {
        if (arith32) res = (double)eval_image_overlap<float>((float)d[0], (float)d[1], (float)d[2], (float)d[3], (float)g[0], (float)g[1], (float)g[2], (float)g[3], -1);
        else {
            res = eval_image_overlap<double>(d[0], d[1], d[2], d[3], g[0], g[1], g[2], g[3], -1);
            if (out32) res = (double)(float)res;               // stored into zeros(dtype=boxes.dtype), eval.py:87
        }
    } else {
        // rotate_iou_gpu_eval casts to float32 first (rotate_iou.py:358-359); the label box is the "query" = rbox1
        const double q[5] = { (double)(float)g[4], (double)(float)g[6], (double)(float)g[7], (double)(float)g[9], (double)(float)g[10] };
        const double b[5] = { (double)(float)d[4], (double)(float)d[6], (double)(float)d[7], (double)(float)d[9], (double)(float)d[10] };
        const double inter = eval_rotated_intersection(q, b);
        if (metric == 1) {
            const double a1 = (double)((float)q[2] * (float)q[3]), a2 = (double)((float)b[2] * (float)b[3]);
            res = (double)(float)(inter / (a1 + a2 - inter));
        } else {
            const float rinc = (float)inter;
            res = arith32 ? eval_d3<float>(d, g, rinc) : eval_d3<double>(d, g, rinc);
        }
    }
    ov[p] = res;
}

struct MatchArgs {
    int second_pass, metric, compute_aos, alpha32, dtdata32;
    int n_img, n_combo;
    long long total_gt, total_dt;
    const long long *dt_off, *gt_off, *ov_off, *dc_off;
    const double *ov, *dt_box, *dt_alpha, *gt_alpha, *dc_box;
    const signed char *ign_gt, *ign_dt;          // [n_cd][total]
    const int *combo_cd; const double *combo_min_overlap;
    const double *thresholds; const int *n_thr;  // [n_combo][41], [n_combo]
    double *match_score;                          // pass 1: [n_combo][total_gt], NaN = label not a true positive
    int *st_tp, *st_fp, *st_fn; double *st_sim;  // pass 2: [n_combo][41][n_img]
};

__global__ void __launch_bounds__(128) kitti_match_kernel(const MatchArgs a) {
    const long long gid = (long long)blockIdx.x * 128 + threadIdx.x;
    const long long per_combo = a.second_pass ? (long long)kEvalSamples * a.n_img : a.n_img;
    if (gid >= per_combo * a.n_combo) return;
    const int combo = (int)(gid / per_combo);
    const long long rem = gid - (long long)combo * per_combo;
    const int t = a.second_pass ? (int)(rem / a.n_img) : 0;
    const int img = (int)(rem - (long long)t * a.n_img);
    if (a.second_pass && t >= a.n_thr[combo]) return;
    const int cd = a.combo_cd[combo];
    const double min_ov = a.combo_min_overlap[combo];
    const double thresh = a.second_pass ? a.thresholds[combo * kEvalSamples + t] : 0.0;
    const long long d0 = a.dt_off[img], g0 = a.gt_off[img];
    const int nd = (int)(a.dt_off[img + 1] - d0), ng = (int)(a.gt_off[img + 1] - g0);
    const signed char *ig = a.ign_gt + (long long)cd * a.total_gt + g0, *id = a.ign_dt + (long long)cd * a.total_dt + d0;
    const double *ov = a.ov + a.ov_off[img];
    unsigned long long taken[kEvalMaxDet / 64];
#pragma unroll
    for (int k = 0; k < kEvalMaxDet / 64; ++k) taken[k] = 0ull;
    auto is_taken = [&](int j) { return (taken[j >> 6] >> (j & 63)) & 1ull; };
    auto take = [&](int j) { taken[j >> 6] |= 1ull << (j & 63); };
    auto below = [&](int j) { return a.second_pass && a.dt_box[(d0 + j) * 12 + 11] < thresh; };
    const double NO_DET = -10000000.0;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    for (int i = 0; i < ng; ++i) {
        if (ig[i] == -1) continue;
        int pick = -1; double best_score = NO_DET, best_ov = 0.0; bool via_ignored = false;
        for (int j = 0; j < nd; ++j) {
            if (id[j] == -1 || is_taken(j) || below(j)) continue;
            const double o = ov[(long long)j * ng + i];
            if (!(o > min_ov)) continue;
            const double sc = a.dt_box[(d0 + j) * 12 + 11];
            if (!a.second_pass) { if (sc > best_score) { pick = j; best_score = sc; } }
            else if (id[j] == 0 && (o > best_ov || via_ignored)) { pick = j; best_score = 1.0; best_ov = o; via_ignored = false; }
            else if (id[j] == 1 && best_score == NO_DET) { pick = j; best_score = 1.0; via_ignored = true; }
        }
        if (best_score == NO_DET) { if (ig[i] == 0) ++fn; }
        else if (ig[i] == 1 || id[pick] == 1) take(pick);
        else {
            ++tp;
            take(pick);
            if (!a.second_pass) a.match_score[(long long)combo * a.total_gt + g0 + i] = a.dt_box[(d0 + pick) * 12 + 11];
            else if (a.compute_aos) {
                const double ga = a.gt_alpha[g0 + i], da = a.dt_alpha[d0 + pick];
                const double delta = a.alpha32 ? (double)((float)ga - (float)da) : ga - da;       // float32 - float32 under numba
                sim += (1.0 + cos(delta)) / 2.0;                 // numba's np.sum: sequential, label order
            }
        }
    }
    if (!a.second_pass) return;
    for (int j = 0; j < nd; ++j) if (!(is_taken(j) || id[j] == -1 || id[j] == 1 || below(j))) ++fp;
    if (a.metric == 0) {
        int stuff = 0;
        for (long long k = a.dc_off[img]; k < a.dc_off[img + 1]; ++k) {
            const double *q = a.dc_box + k * 4;
            for (int j = 0; j < nd; ++j) {
                if (is_taken(j) || id[j] == -1 || id[j] == 1 || below(j)) continue;
                const double *d = a.dt_box + (d0 + j) * 12;
                double o = eval_image_overlap<double>(d[0], d[1], d[2], d[3], q[0], q[1], q[2], q[3], 0);
                if (a.dtdata32) o = (double)(float)o;
                if (o > min_ov) { take(j); ++stuff; }
            }
        }
        fp -= stuff;
    }
    if (a.compute_aos && !(tp > 0 || fp > 0)) sim = -1.0;
    const long long o = ((long long)combo * kEvalSamples + t) * a.n_img + img;
    a.st_tp[o] = tp; a.st_fp[o] = fp; a.st_fn[o] = fn; a.st_sim[o] = sim;
}

__global__ void __launch_bounds__(64) kitti_reduce_kernel(int n_img, int n_combo, const int *n_thr, const int *st_tp, const int *st_fp,
                                                          const int *st_fn, const double *st_sim, double *pr) {
    const int gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= n_combo * kEvalSamples) return;
    const int combo = gid / kEvalSamples, t = gid - combo * kEvalSamples;
    double tp = 0.0, fp = 0.0, fn = 0.0, sim = 0.0;
    if (t < n_thr[combo]) {
        const long long o = (long long)gid * n_img;
        for (int i = 0; i < n_img; ++i) {                        // image order, as fused_compute_statistics accumulates
            tp += (double)st_tp[o + i]; fp += (double)st_fp[o + i]; fn += (double)st_fn[o + i];
            const double s = st_sim[o + i];
            if (s != -1.0) sim += s;
        }
    }
    pr[gid * 4 + 0] = tp; pr[gid * 4 + 1] = fp; pr[gid * 4 + 2] = fn; pr[gid * 4 + 3] = sim;
}
