// noc_decode_kernel.inc — K2, the NOC head's post-processing (included by monorun_pnp.hip inside its anonymous namespace, ahead of PnpArgs, which
// embeds DecodeArgs): the RoIAlign bin samplers it shares with mr_roi_align_avg, the specified exp / log, the decode (also K1's load stage), both kernels.
// ------------------------------------------------------------------------------------------------
// K2: fused NOC-head post-processing.  One thread per RoI pixel; every read of all_pred is a coalesced
// row of the selected channel, every write a coalesced row of a channel-planar output map.
//   R9  flip/class channel pick   fcn_noc_decoder.py:225-267  (integer indexing, bit-exact)
//   R10 dim + NOC decode          multiclass_norm_dim_coder.py:28-36, noc_coder.py:50-73
//   R11 log-std decode            distance_invar_proj_error_coder.py:39-60 (distance=None)
//   R8  istd, RANSAC threshold    uncert_prop_pnp_optimizer.py:73,86-88
//   R12 RoI bin-centre grid       roi_align(coord_2d, ..., 'avg', aligned=True), interior analytic form
// fp32 with unfused multiply-adds, i.e. the rounding sequence of the reference's elementwise torch ops.
// The per-object / per-pixel arithmetic is shared with the fused path of the PnP kernel (decoded maps
// written straight into its LDS tile, never to HBM).
struct DecodeArgs {
    const void *all_pred; int pred_dtype;      // head output: MR_F32, MR_F16 or MR_BF16 (autocast pipelines); decoded in fp32
    const long long *labels; const uint8_t *flip; const float *dim, *dim_var, *rois;
    int B, C, agnostic, h, w;
    const float *dim_means, *dim_stds, *noc_means, *noc_stds;     // device pointers: (C,3), (C,3), (3), (3)
    float k_epi, k_sd2, sd_sq, std_scale, ratio; int has_var;
    float *c2d, *istd, *c3d, *dims, *dims_var, *thr;
    const float *map2d; int map_h, map_w;      // optional coord_2d map (2, H, W): exact RoIAlign sampling instead of the analytic grid
    unsigned w_magic;                          // floor((2^32 - 1) / w) + 1 (0 when w == 1 or h * w >= 65536): row index p / w == __umulhi(p, w_magic), decode_pixel_pair
};

// RoIAlign forward, average pooling (mmcv.ops.roi_align: the published Detectron/mmcv algorithm, mmcv 1.2.1
// roi_align_cuda_kernel.cuh — third-party, not in the reference tree): bilinear taps with mmcv's border rules
// (a sample more than one pixel outside contributes 0; otherwise it is clamped into [0, size-1]).
__device__ __forceinline__ float roi_bilinear(const float *in, int H, int W, float y, float x) {
#pragma clang fp contract(off)
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) return 0.0f;
    if (y <= 0.0f) y = 0.0f;
    if (x <= 0.0f) x = 0.0f;
    int y_low = (int)y, x_low = (int)x, y_high, x_high;
    if (y_low >= H - 1) { y_high = y_low = H - 1; y = (float)y_low; } else y_high = y_low + 1;
    if (x_low >= W - 1) { x_high = x_low = W - 1; x = (float)x_low; } else x_high = x_low + 1;
    const float ly = y - (float)y_low, lx = x - (float)x_low, hy = 1.0f - ly, hx = 1.0f - lx;
    const float v1 = in[y_low * W + x_low], v2 = in[y_low * W + x_high], v3 = in[y_high * W + x_low], v4 = in[y_high * W + x_high];
    const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
    return w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
}

// one output bin (ph, pw) of one channel; roi = x1 y1 x2 y2 already multiplied by spatial_scale
__device__ __forceinline__ float roi_align_avg_bin(const float *in, int H, int W, float x1, float y1, float x2, float y2,
                                                   int ph, int pw, int out_h, int out_w, int sampling_ratio, int aligned) {
#pragma clang fp contract(off)
    const float off = aligned ? 0.5f : 0.0f;
    const float sw = x1 - off, sh = y1 - off;
    float rw = (x2 - off) - sw, rh = (y2 - off) - sh;
    if (!aligned) { rw = fmaxf(rw, 1.0f); rh = fmaxf(rh, 1.0f); }
    const float bh = rh / (float)out_h, bw = rw / (float)out_w;
    const int gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)out_h);
    const int gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)out_w);
    const float count = (float)max(gh * gw, 1);
    float acc = 0.0f;
    for (int iy = 0; iy < gh; ++iy) {
        const float y = sh + (float)ph * bh + ((float)iy + 0.5f) * bh / (float)gh;
        for (int ix = 0; ix < gw; ++ix) {
            const float x = sw + (float)pw * bw + ((float)ix + 0.5f) * bw / (float)gw;
            acc += roi_bilinear(in, H, W, y, x);
        }
    }
    return acc / count;
}

// The same rules in parts, for the multi-level extractor (roi_extract_kernel.inc), which computes a RoI's sample geometry once and reuses it for
// every channel, and transposes it in its backward: roi_bilinear = roi_axis_tap in y and in x + roi_blend; roi_align_avg_bin = roi_geom +
// roi_sample_coord + that.  Operation for operation the arithmetic above (tests/test_gpu_roi_extract.py compares the two bit for bit).  The two
// functions above keep their own text: expressed through the parts they moved the code of 17 tuned kernels (the fused PnP instantiations, K2,
// roi_align_avg_kernel; tools/isa_diff.sh), as the folds of HISTORY.md round 12 did.
// One axis of a bilinear sample (the y rule and the x rule are the same): `dead` when the coordinate is more than a pixel outside [0, size);
// else the two taps lo, hi (equal in the last row / column) and their weights h = 1 - l, l.
struct RoiTap { int lo, hi; float l, h; };
__device__ __forceinline__ bool roi_axis_tap(float v, int size, RoiTap &t) {
#pragma clang fp contract(off)
    if (v < -1.0f || v > (float)size) return true;
    if (v <= 0.0f) v = 0.0f;
    t.lo = (int)v;
    if (t.lo >= size - 1) { t.hi = t.lo = size - 1; v = (float)t.lo; } else t.hi = t.lo + 1;
    t.l = v - (float)t.lo; t.h = 1.0f - t.l;
    return false;
}
// the four taps of one sample of one channel, blended: the order of the products and of the sum is the definition
__device__ __forceinline__ float roi_blend(const float *in, int W, const RoiTap &ty, const RoiTap &tx) {
#pragma clang fp contract(off)
    const float v1 = in[ty.lo * W + tx.lo], v2 = in[ty.lo * W + tx.hi], v3 = in[ty.hi * W + tx.lo], v4 = in[ty.hi * W + tx.hi];
    const float w1 = ty.h * tx.h, w2 = ty.h * tx.l, w3 = ty.l * tx.h, w4 = ty.l * tx.l;
    return w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4;
}
// The per-RoI terms of the pooling; roi = x1 y1 x2 y2 already multiplied by spatial_scale.  gh, gw: the sample grid of a bin (<= 0: no
// sample), count the divisor.  At sampling_ratio 0 the grid is (int)ceilf(rh / out_h): the caller bounds it where the RoI is not trusted.
struct RoiGeom { float sw, sh, rw, rh, bw, bh, count; int gw, gh; };
__device__ __forceinline__ RoiGeom roi_geom(float x1, float y1, float x2, float y2, int out_h, int out_w, int sampling_ratio, int aligned) {
#pragma clang fp contract(off)
    RoiGeom g;
    const float off = aligned ? 0.5f : 0.0f;
    g.sw = x1 - off; g.sh = y1 - off;
    g.rw = (x2 - off) - g.sw; g.rh = (y2 - off) - g.sh;
    if (!aligned) { g.rw = fmaxf(g.rw, 1.0f); g.rh = fmaxf(g.rh, 1.0f); }
    g.bh = g.rh / (float)out_h; g.bw = g.rw / (float)out_w;
    g.gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.rh / (float)out_h);
    g.gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(g.rw / (float)out_w);
    g.count = (float)max(g.gh * g.gw, 1);
    return g;
}
// the coordinate of sample i of the g of bin p along one axis (start: sh or sw, bin: bh or bw)
__device__ __forceinline__ float roi_sample_coord(float start, float bin, int p, int i, int g) {
#pragma clang fp contract(off)
    return start + (float)p * bin + ((float)i + 0.5f) * bin / (float)g;
}

// exp / log of the istd chain, SPECIFIED (not library calls): the decoded istd feeds a bit-exact threshold (the istd inlier
// mask, pnp_uncert_cpu.py:164-168), so its last bit must not depend on which libm / device library computed it.  Classical
// single-precision algorithms (Cephes expf / logf: Cody-Waite reduction with the two-part ln 2, degree-5 / degree-8
// polynomials) written as a fixed sequence of IEEE float32 multiplications and additions — no fma, no contraction — which the
// test infrastructure restates operation for operation with numpy float32 arithmetic (spec_expf / spec_logf there).  Error <= 1 ulp.
__device__ __forceinline__ float mr_expf(float x) {
#pragma clang fp contract(off)
    if (x > 88.72283935546875f) return __int_as_float(0x7f800000);
    if (x < -103.0f) return 0.0f;
    const float kf = rintf(x * 1.44269504088896341f);
    float r = x - kf * 0.693359375f;
    r = r - kf * -2.12194440e-4f;
    const float z = r * r;
    float p = 1.9875691500E-4f * r + 1.3981999507E-3f;
    p = p * r + 8.3334519073E-3f;
    p = p * r + 4.1665795894E-2f;
    p = p * r + 1.6666665459E-1f;
    p = p * r + 5.0000001201E-1f;
    float y = p * z + r;
    y = y + 1.0f;
    return ldexpf(y, (int)kf);                 // NaN in -> NaN out (both range tests are false)
}
__device__ __forceinline__ float mr_logf(float x) {
#pragma clang fp contract(off)
    if (!(x > 0.0f)) return x == 0.0f ? -__int_as_float(0x7f800000) : __int_as_float(0x7fc00000);
    if (x == __int_as_float(0x7f800000)) return x;
    int e;
    float m = frexpf(x, &e);
    if (m < 0.707106781186547524f) { e -= 1; m = m + m - 1.0f; } else m = m - 1.0f;
    const float z = m * m;
    float p = 7.0376836292E-2f * m - 1.1514610310E-1f;
    p = p * m + 1.1676998740E-1f;
    p = p * m - 1.2420140846E-1f;
    p = p * m + 1.4249322787E-1f;
    p = p * m - 1.6668057665E-1f;
    p = p * m + 2.0000714765E-1f;
    p = p * m - 2.4999993993E-1f;
    p = p * m + 3.3333331174E-1f;
    const float fe = (float)e;
    float y = m * (z * p);
    y = y + -2.12194440e-4f * fe;
    y = y - 0.5f * z;
    const float zz = m + y;
    return zz + 0.693359375f * fe;
}

struct DecodeObj { float dm[3], dv[3], nm[3], ns[3]; float x1, y1, x2, y2, su, sv, thr; long long base; int ch_noc, ch_ls; };   // base: element offset of the object

__device__ __forceinline__ float pred_at(const DecodeArgs &a, long long i) {
    if (a.pred_dtype == MR_F32) return ((const float *)a.all_pred)[i];
    if (a.pred_dtype == MR_F16) return __half2float(((const __half *)a.all_pred)[i]);
    return __uint_as_float((unsigned)((const unsigned short *)a.all_pred)[i] << 16);            // bfloat16
}

// WITH_ROI = false: the class / flip channel pick and the dim decode only — what the training decode needs (noc_decode_train_kernel.inc); a.rois is not read
template <bool WITH_ROI = true>
__device__ __forceinline__ void decode_object(const DecodeArgs &a, int b, DecodeObj &o) {
#pragma clang fp contract(off)
    const int hw = a.h * a.w;
    const int lab = (int)a.labels[b];
    const int c = a.agnostic ? 0 : lab;
    const int f = a.flip[b] ? 1 : 0;
    const int Cn = a.agnostic ? 1 : a.C;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sd = a.dim_stds[lab * 3 + k];
        o.dm[k] = a.dim[b * 3 + k] * sd + a.dim_means[lab * 3 + k];
        o.dv[k] = a.has_var ? a.dim_var[b * 3 + k] * (sd * sd) : 0.0f;
        o.nm[k] = a.noc_means[k]; o.ns[k] = a.noc_stds[k];
    }
    if constexpr (WITH_ROI) {
    const float x1 = a.rois[b * 4 + 0], y1 = a.rois[b * 4 + 1], x2 = a.rois[b * 4 + 2], y2 = a.rois[b * 4 + 3];
    o.x1 = x1; o.y1 = y1;
    o.su = (x2 - x1) / (float)a.w; o.sv = (y2 - y1) / (float)a.h;
    o.x2 = x2; o.y2 = y2;
    float v_last, v_first;
    if (a.map2d) {      // x2d[:, 1, -1, 0] - x2d[:, 1, 0, 0] of the sampled map (uncert_prop_pnp_optimizer.py:86-88)
        const float *mv = a.map2d + (long long)a.map_h * a.map_w;
        v_last = roi_align_avg_bin(mv, a.map_h, a.map_w, x1, y1, x2, y2, a.h - 1, 0, a.h, a.w, 0, 1);
        v_first = roi_align_avg_bin(mv, a.map_h, a.map_w, x1, y1, x2, y2, 0, 0, a.h, a.w, 0, 1);
    } else {
        v_last = (y1 - 0.5f) + ((float)(a.h - 1) + 0.5f) * o.sv; v_first = (y1 - 0.5f) + 0.5f * o.sv;
    }
    o.thr = a.ratio * (v_last - v_first);
    }
    o.base = (long long)b * (2 * Cn * 5) * hw;
    o.ch_noc = f * 5 * Cn + 3 * c; o.ch_ls = f * 5 * Cn + 3 * Cn + 2 * c;
}

// (the scalar form, textually what the fused PnP kernel has been tuned around: its code must not move — tools/isa_diff.sh)
__device__ __forceinline__ void decode_pixel(const DecodeArgs &a, const DecodeObj &o, int p, float (&c2d)[2], float (&istd)[2], float (&c3d)[3]) {
#pragma clang fp contract(off)
    const int hw = a.h * a.w;
    const int py = p / a.w, px = p - py * a.w;
    float xv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float noc = pred_at(a, o.base + (long long)(o.ch_noc + k) * hw + p);
        const float part = noc * o.ns[k] + o.nm[k];
        c3d[k] = part * o.dm[k];
        xv[k] = o.dv[k] * (part * part);
    }
    const float v2[2] = { 0.5f * (xv[0] + xv[2]), xv[1] };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float ls = pred_at(a, o.base + (long long)(o.ch_ls + k) * hw + p);
        float lspx;
        if (a.has_var) lspx = 0.5f * mr_logf((v2[k] * a.k_epi + mr_expf(2.0f * ls) * a.k_sd2) / a.sd_sq);
        else lspx = ls + 0.0f;                                    // log(sd / sd)
        istd[k] = mr_expf(-lspx) / a.std_scale;
    }
    if (a.map2d) {      // roi_align(coord_2d, rois, (h, w), 1.0, 0, 'avg', True)   (monorun_roi_head.py:521-523)
        c2d[0] = roi_align_avg_bin(a.map2d, a.map_h, a.map_w, o.x1, o.y1, o.x2, o.y2, py, px, a.h, a.w, 0, 1);
        c2d[1] = roi_align_avg_bin(a.map2d + (long long)a.map_h * a.map_w, a.map_h, a.map_w, o.x1, o.y1, o.x2, o.y2, py, px, a.h, a.w, 0, 1);
    } else {            // interior analytic form: the bin centre of an identity coordinate map
        c2d[0] = (o.x1 - 0.5f) + ((float)px + 0.5f) * o.su;
        c2d[1] = (o.y1 - 0.5f) + ((float)py + 0.5f) * o.sv;
    }
}

// the same arithmetic from five head-channel VALUES (the vector kernel loads them four pixels at a time); analytic grid only
__device__ __forceinline__ void decode_pixel_vals(const DecodeArgs &a, const DecodeObj &o, int p, const float (&nocv)[3], const float (&lsv)[2],
                                                  float (&c2d)[2], float (&istd)[2], float (&c3d)[3]) {
#pragma clang fp contract(off)
    const int py = p / a.w, px = p - py * a.w;
    float xv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float part = nocv[k] * o.ns[k] + o.nm[k];
        c3d[k] = part * o.dm[k];
        xv[k] = o.dv[k] * (part * part);
    }
    const float v2[2] = { 0.5f * (xv[0] + xv[2]), xv[1] };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float ls = lsv[k];
        float lspx;
        if (a.has_var) lspx = 0.5f * mr_logf((v2[k] * a.k_epi + mr_expf(2.0f * ls) * a.k_sd2) / a.sd_sq);
        else lspx = ls + 0.0f;                                    // log(sd / sd)
        istd[k] = mr_expf(-lspx) / a.std_scale;
    }
    if (a.map2d) {      // roi_align(coord_2d, rois, (h, w), 1.0, 0, 'avg', True)   (monorun_roi_head.py:521-523)
        c2d[0] = roi_align_avg_bin(a.map2d, a.map_h, a.map_w, o.x1, o.y1, o.x2, o.y2, py, px, a.h, a.w, 0, 1);
        c2d[1] = roi_align_avg_bin(a.map2d + (long long)a.map_h * a.map_w, a.map_h, a.map_w, o.x1, o.y1, o.x2, o.y2, py, px, a.h, a.w, 0, 1);
    } else {            // interior analytic form: the bin centre of an identity coordinate map
        c2d[0] = (o.x1 - 0.5f) + ((float)px + 0.5f) * o.su;
        c2d[1] = (o.y1 - 0.5f) + ((float)py + 0.5f) * o.sv;
    }
}

__global__ void __launch_bounds__(256) noc_decode_kernel(const DecodeArgs a) {
    const int hw = a.h * a.w;
    const int bpo = (hw + 255) >> 8;                   // blocks per object; 1-D grid: B * bpo <= 2^31 - 1
    const int b = blockIdx.x / bpo;
    const int p = (blockIdx.x - b * bpo) * 256 + threadIdx.x;
    DecodeObj o;
    decode_object(a, b, o);
    if (p == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.dims) a.dims[b * 3 + k] = o.dm[k];
            if (a.dims_var && a.has_var) a.dims_var[b * 3 + k] = o.dv[k];
        }
        if (a.thr) a.thr[b] = o.thr;
    }
    if (p >= hw) return;
    float c2d[2], istd[2], c3d[3];
    decode_pixel(a, o, p, c2d, istd, c3d);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.c3d[((long long)b * 3 + k) * hw + p] = c3d[k];
#pragma unroll
    for (int k = 0; k < 2; ++k) { a.istd[((long long)b * 2 + k) * hw + p] = istd[k]; a.c2d[((long long)b * 2 + k) * hw + p] = c2d[k]; }
}

// Two-pixel forms of the same arithmetic for the vector kernel: every multiplication and addition of the specified sequences acts on
// a PAIR of pixels (v_pk_mul_f32 / v_pk_add_f32: one instruction, two IEEE float32 results, each bit-identical to the scalar
// operation), the special cases become selects after the common path.  mr_expf / mr_logf / decode_pixel_vals stay the definition.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// CHECKED = false: the common path only — the caller is told (`special`) when an argument falls into a special case and redoes the
// work with the checked form; on ordinary inputs this drops the compares and selects (~ 10 % of the vector kernel's instructions).
template <bool CHECKED = true>
__device__ __forceinline__ f32x2 mr_expf2(f32x2 x, bool *special = nullptr) {
#pragma clang fp contract(off)
    f32x2 kf;
    kf.x = rintf(x.x * 1.44269504088896341f); kf.y = rintf(x.y * 1.44269504088896341f);
    f32x2 r = x - kf * 0.693359375f;
    r = r - kf * -2.12194440e-4f;
    const f32x2 z = r * r;
    f32x2 p = 1.9875691500E-4f * r + 1.3981999507E-3f;
    p = p * r + 8.3334519073E-3f;
    p = p * r + 4.1665795894E-2f;
    p = p * r + 1.6666665459E-1f;
    p = p * r + 5.0000001201E-1f;
    f32x2 y = p * z + r;
    y = y + 1.0f;
    f32x2 o;
    o.x = ldexpf(y.x, (int)kf.x); o.y = ldexpf(y.y, (int)kf.y);
    if constexpr (CHECKED) {
        o.x = x.x > 88.72283935546875f ? __int_as_float(0x7f800000) : (x.x < -103.0f ? 0.0f : o.x);
        o.y = x.y > 88.72283935546875f ? __int_as_float(0x7f800000) : (x.y < -103.0f ? 0.0f : o.y);
    } else {
        // conservative: |x + 7.14| > 95.8 holds for every x > 88.72283935546875 and every x < -103 (and for a sliver inside the range: a
        // false alarm only costs the redo); a NaN is not special — it goes through the same arithmetic in the checked form
        *special = *special || (fabsf(x.x + 7.14f) > 95.8f) || (fabsf(x.y + 7.14f) > 95.8f);
    }
    return o;
}
template <bool CHECKED = true>
__device__ __forceinline__ f32x2 mr_logf2(f32x2 x, bool *special = nullptr) {
#pragma clang fp contract(off)
    int e0, e1;
    f32x2 m;
    m.x = frexpf(x.x, &e0); m.y = frexpf(x.y, &e1);
    const bool lo0 = m.x < 0.707106781186547524f, lo1 = m.y < 0.707106781186547524f;
    e0 -= lo0 ? 1 : 0; e1 -= lo1 ? 1 : 0;
    const f32x2 m2 = m + m - 1.0f, m1 = m - 1.0f;
    m.x = lo0 ? m2.x : m1.x; m.y = lo1 ? m2.y : m1.y;
    const f32x2 z = m * m;
    f32x2 p = 7.0376836292E-2f * m - 1.1514610310E-1f;
    p = p * m + 1.1676998740E-1f;
    p = p * m - 1.2420140846E-1f;
    p = p * m + 1.4249322787E-1f;
    p = p * m - 1.6668057665E-1f;
    p = p * m + 2.0000714765E-1f;
    p = p * m - 2.4999993993E-1f;
    p = p * m + 3.3333331174E-1f;
    f32x2 fe;
    fe.x = (float)e0; fe.y = (float)e1;
    f32x2 y = m * (z * p);
    y = y + -2.12194440e-4f * fe;
    y = y - 0.5f * z;
    const f32x2 zz = m + y;
    f32x2 o = zz + 0.693359375f * fe;
    const float inf = __int_as_float(0x7f800000), nan = __int_as_float(0x7fc00000);
    if constexpr (CHECKED) {
        o.x = !(x.x > 0.0f) ? (x.x == 0.0f ? -inf : nan) : (x.x == inf ? x.x : o.x);
        o.y = !(x.y > 0.0f) ? (x.y == 0.0f ? -inf : nan) : (x.y == inf ? x.y : o.y);
    } else {
        *special = *special || !(x.x > 0.0f) || !(x.y > 0.0f) || x.x == inf || x.y == inf;      // zero, negative, NaN, +inf
    }
    return o;
}
// pixels p and p + 1 of one object row-major (p even, same row: w is even whenever h * w % 4 == 0 ... not required: px / py per pixel)
// x / c for a wave-uniform float32 c, correctly rounded like the IEEE division it replaces, in 3 instructions instead of ~12: the
// quotient is formed in float64 as x * RN64(1 / c) (relative error < 2^-52) and rounded to float32 once.  A float32 quotient of two
// float32 numbers is never closer than 2^-49 (relative) to a rounding boundary — with X, C the 24-bit significands and M the odd 25-bit
// significand of a midpoint, X 2^s - M C is a non-zero integer — so that single rounding lands on the IEEE result; zeros, infinities,
// NaNs, c = 0, overflow and float32 denormals go through the float64 product and the conversion unchanged.  rc = 1.0 / (double)c.
__device__ __forceinline__ float div_by_uniform(float x, double rc) { return (float)((double)x * rc); }

// w_magic = floor((2^32 - 1) / w) + 1: p / w == __umulhi(p, w_magic) for p, w < 2^16 (the error of the product is p (w_magic w - 2^32)
// / (w 2^32) < p / 2^32 < 1 / w) — the two integer divisions per pixel pair were ~ 12 % of the kernel's instructions
// The two pixels are p and p + 1 (the vector decode kernel), or p and pb (the fused kernel's load stage: a lane's pixels are a stride apart).
// CHECKED = false needs `special` (it is written); CHECKED = true ignores it.
template <bool CHECKED = true, bool ADJACENT = true>
__device__ __forceinline__ void decode_pixel_pair(const DecodeArgs &a, const DecodeObj &o, int p, const f32x2 (&nocv)[3], const f32x2 (&lsv)[2],
                                                  f32x2 (&c2d)[2], f32x2 (&istd)[2], f32x2 (&c3d)[3], double rc_sd_sq, double rc_std_scale, unsigned w_magic,
                                                  bool *special = nullptr, int pb = 0) {
#pragma clang fp contract(off)
    f32x2 xv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const f32x2 part = nocv[k] * o.ns[k] + o.nm[k];
        c3d[k] = part * o.dm[k];
        xv[k] = o.dv[k] * (part * part);
    }
    const f32x2 v2[2] = { 0.5f * (xv[0] + xv[2]), xv[1] };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const f32x2 ls = lsv[k];
        f32x2 lspx;
        if (a.has_var) {
            const f32x2 num = v2[k] * a.k_epi + mr_expf2<CHECKED>(2.0f * ls, special) * a.k_sd2;
            f32x2 q;
            q.x = div_by_uniform(num.x, rc_sd_sq); q.y = div_by_uniform(num.y, rc_sd_sq);
            lspx = 0.5f * mr_logf2<CHECKED>(q, special);
        } else lspx = ls + 0.0f;                                  // log(sd / sd)
        const f32x2 ex = mr_expf2<CHECKED>(-lspx, special);
        istd[k].x = div_by_uniform(ex.x, rc_std_scale); istd[k].y = div_by_uniform(ex.y, rc_std_scale);
    }
    const int py0 = (int)__umulhi((unsigned)p, w_magic), px0 = p - py0 * a.w;
    int py1, px1;
    if constexpr (ADJACENT) {
        const bool wrap = px0 + 1 == a.w;                         // pixel p + 1 starts the next row
        py1 = wrap ? py0 + 1 : py0; px1 = wrap ? 0 : px0 + 1;
    } else { py1 = (int)__umulhi((unsigned)pb, w_magic); px1 = pb - py1 * a.w; }
    f32x2 fx, fy;
    fx.x = (float)px0; fx.y = (float)px1; fy.x = (float)py0; fy.y = (float)py1;
    c2d[0] = (o.x1 - 0.5f) + (fx + 0.5f) * o.su;
    c2d[1] = (o.y1 - 0.5f) + (fy + 0.5f) * o.sv;
}

// K2, vector form: one thread per FOUR consecutive RoI pixels of one object — five 16-byte loads of the selected head channels,
// seven 16-byte NON-TEMPORAL stores of the decoded channels.  One workgroup per object (grid = B).  Same per-pixel arithmetic as the
// scalar kernel above (two pixels per packed instruction), hence bit-identical outputs.  What bounds it, as measured (per-wave 100 MHz
// stamps, profiles/r04_k2_timeline.txt, r04_k2_store_policy.txt):
//   * a wave has its parameters 2.0 us after it starts (three dependent rounds of loads), its pixel loads out 0.9 us later, the data
//     0.5 us later — the pixel data is NOT what is late —, its arithmetic done after another 3.1 us; waves start within 0.7 us;
//   * with plain stores the profiler counted 2 - 3 us more than the last wave's end: the write-back of the 22 MB of outputs from L2 when
//     the dispatch ends.  Non-temporal stores send them on during the launch (12.1 - 12.7 -> 10.2 - 11.9 us);
//   * from there the launch is instruction-issue-bound, and cuts of the stream count: the object's last wave on pixel pairs, the row
//     index by multiplication, the exp / log sequences on their common path first (809 -> 620 VALU instructions per wave; 9.5 - 9.8 us
//     per launch issued back to back = 0.49 - 0.51 of 8 TB/s, an isolated launch 8.0 us).
// Measured and not kept (same files; HISTORY.md): a persistent software-pipelined form, 128- and 64-thread workgroups, caps on the
// resident workgroups, a grouped form (several objects per workgroup, lanes numbered through their quads), non-temporal loads, the class
// rows fetched ahead of the label, the pixel loads issued ahead of the other parameters, starting the waves of a SIMD apart, Horner
// chains interleaved across four pixels.  Requires fp32 head output, h * w % 4 == 0 and < 65536, no coord_2d map (the launcher falls
// back to the scalar kernel otherwise).
template <int THREADS, int TRIPS>
__global__ void __launch_bounds__(THREADS) noc_decode_kernel_x4(const DecodeArgs a, int quads_per_obj) {
    // one workgroup per object: the object index is wave-uniform, so its parameters (label, flip, dims, RoI, coder constants — two
    // dependent rounds of loads) are fetched through the scalar cache once per wave instead of once per lane.  A thread takes up
    // to TRIPS pixel quads (q = t, t + THREADS, ...): all their loads are issued before the first quad is decoded, so the
    // arithmetic of one quad (the specified exp / log sequences and IEEE divisions: ~300 instructions per pixel) overlaps the
    // loads of the next and the stores of the previous one.
    const int b = blockIdx.x;
    const int hw = a.h * a.w;
    const unsigned w_magic = a.w_magic;
    DecodeObj o;
    decode_object(a, b, o);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (a.dims) a.dims[b * 3 + k] = o.dm[k];
            if (a.dims_var && a.has_var) a.dims_var[b * 3 + k] = o.dv[k];
        }
        if (a.thr) a.thr[b] = o.thr;
    }
    const float *ap = (const float *)a.all_pred;
    const double rc_sd_sq = 1.0 / (double)a.sd_sq, rc_std_scale = 1.0 / (double)a.std_scale;      // div_by_uniform
    if constexpr (TRIPS == 1) {
        // The last wave of an object owns only the quads left over (28x28: 4 of 196) and would still issue the whole two-pairs-per-lane
        // instruction stream for them.  With at most 32 quads left it works on PAIRS instead: lane l takes pixels (2l, 2l + 1) of the
        // wave's range — one pass through the same packed arithmetic, half the instructions, 8-byte loads and stores.
        const int w0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * 64;      // first quad of this wave
        const int nq = quads_per_obj - w0;
        if (nq > 0 && nq <= 32) {
            const int l = threadIdx.x & 63;
            if (l < 2 * nq) {
                const int p0 = 4 * w0 + 2 * l;
                typedef float f32x2v __attribute__((ext_vector_type(2)));
                f32x2 noc[3], ls[2], c2[2], w2[2], c3[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { const float2 v = *(const float2 *)(ap + o.base + (long long)(o.ch_noc + k) * hw + p0); noc[k].x = v.x; noc[k].y = v.y; }
#pragma unroll
                for (int k = 0; k < 2; ++k) { const float2 v = *(const float2 *)(ap + o.base + (long long)(o.ch_ls + k) * hw + p0); ls[k].x = v.x; ls[k].y = v.y; }
                bool special = false;
                decode_pixel_pair<false>(a, o, p0, noc, ls, c2, w2, c3, rc_sd_sq, rc_std_scale, w_magic, &special);
                if (special) decode_pixel_pair<true>(a, o, p0, noc, ls, c2, w2, c3, rc_sd_sq, rc_std_scale, w_magic);
                auto st2 = [](float *dst, f32x2 v) { __builtin_nontemporal_store(f32x2v{ v.x, v.y }, (f32x2v *)dst); };
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    st2(a.c2d + ((long long)b * 2 + k) * hw + p0, c2[k]);
                    st2(a.istd + ((long long)b * 2 + k) * hw + p0, w2[k]);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) st2(a.c3d + ((long long)b * 3 + k) * hw + p0, c3[k]);
            }
            return;
        }
    }
    for (int q0 = threadIdx.x; q0 < quads_per_obj; q0 += THREADS * TRIPS) {
        float4 in[TRIPS][5];
#pragma unroll
        for (int t = 0; t < TRIPS; ++t) {
            const int q = q0 + t * THREADS;
            if (q < quads_per_obj) {
#pragma unroll
                for (int k = 0; k < 3; ++k) in[t][k] = *(const float4 *)(ap + o.base + (long long)(o.ch_noc + k) * hw + 4 * q);
#pragma unroll
                for (int k = 0; k < 2; ++k) in[t][3 + k] = *(const float4 *)(ap + o.base + (long long)(o.ch_ls + k) * hw + 4 * q);
            }
        }
#pragma unroll
        for (int t = 0; t < TRIPS; ++t) {
            const int q = q0 + t * THREADS;
            if (q >= quads_per_obj) break;
            const int p0 = 4 * q;
            float out[7][4];
            // pixel pairs (p0, p0 + 1), (p0 + 2, p0 + 3): packed float32 arithmetic.  First the common path of the specified exp / log
            // sequences (no range tests, no selects); a lane that met a special input redoes its quad with the checked forms.
            auto quad = [&](auto checked, bool *special) {
                constexpr bool CHECKED = decltype(checked)::value;
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    f32x2 noc[3], ls[2], c2[2], w2[2], c3[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { noc[k].x = ((const float *)&in[t][k])[j]; noc[k].y = ((const float *)&in[t][k])[j + 1]; }
#pragma unroll
                    for (int k = 0; k < 2; ++k) { ls[k].x = ((const float *)&in[t][3 + k])[j]; ls[k].y = ((const float *)&in[t][3 + k])[j + 1]; }
                    decode_pixel_pair<CHECKED>(a, o, p0 + j, noc, ls, c2, w2, c3, rc_sd_sq, rc_std_scale, w_magic, special);
                    out[0][j] = c2[0].x; out[0][j + 1] = c2[0].y; out[1][j] = c2[1].x; out[1][j + 1] = c2[1].y;
                    out[2][j] = w2[0].x; out[2][j + 1] = w2[0].y; out[3][j] = w2[1].x; out[3][j + 1] = w2[1].y;
#pragma unroll
                    for (int k = 0; k < 3; ++k) { out[4 + k][j] = c3[k].x; out[4 + k][j + 1] = c3[k].y; }
                }
            };
            bool special = false;
            quad(std::false_type{}, &special);
            if (special) quad(std::true_type{}, nullptr);
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            // NON-TEMPORAL stores (`global_store_dwordx4 ... nt`): the 22 MB a launch writes are not kept in L2, so the write-back at the end
            // of the dispatch has little left to do: 10.2 - 11.3 us per launch against 12.1 - 12.7 us with plain stores (300 launches each way,
            // alternating; `sc0 sc1` write-through stores give the same, non-temporal LOADS nothing: profiles/r04_k2_store_policy.txt)
            auto st4 = [](float *dst, const float (&v)[4]) { __builtin_nontemporal_store(f32x4{ v[0], v[1], v[2], v[3] }, (f32x4 *)dst); };
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                st4(a.c2d + ((long long)b * 2 + k) * hw + p0, out[k]);
                st4(a.istd + ((long long)b * 2 + k) * hw + p0, out[2 + k]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) st4(a.c3d + ((long long)b * 3 + k) * hw + p0, out[4 + k]);
        }
    }
}
