// noc_decode_train_kernel.inc — N8, the NOC head's TRAINING decode (included by monorun_pnp.hip inside its anonymous namespace, after
// noc_decode_kernel.inc, whose DecodeArgs / DecodeObj / decode_object / pred_at / mr_expf / mr_logf it uses, and after pnp_kernel.inc
// for wave_allreduce): the chain from the head's conv_final output to coords_3d and the pixel log-std of forward_train
// (monorun_roi_head.py:189-217, :374-394), forward and backward.
//   slice           fcn_noc_decoder.py:225-267                    K2's ch_noc / ch_ls
//   dim decode      multiclass_norm_dim_coder.py:28-36            dims = dim sigma_c + mu_c, dims_var = dim_var sigma_c^2
//   NOC decode      noc_coder.py:50-73 (part_var = None)          part = noc s + m, coords_3d = part dims, coords_3d_var = dims_var part^2
//   decode_logstd   distance_invar_proj_error_coder.py:39-60      d = clamp(distance, min) or sd:
//                                                                   q = (var2d k_epi + exp(2 ls) sd^2) / d^2, px = 0.5 log q   (with variance)
//                                                                   px = ls + log(sd / d)                                      (without)
// fp32 with unfused multiply-adds in K2's operation order: coords_3d, dims and dims_var are bit-identical to noc_decode's, and with
// distances = NULL the pixel log-std is the one K2 turns into its istd.
struct DecodeTrainArgs {
    DecodeArgs d;                              // the head output, labels, flip, dim, dim_var, coder constants; outputs c3d, dims, dims_var (rois, c2d, istd, thr unused)
    const float *distances;                    // (n) or NULL: the reference distance sd
    float dist_min, sdf;                       // distance_min and sd = ref_length ref_focal_y target_std, both as fp32
    float *noc, *ls, *c3d_var, *lspx;          // forward outputs (n, 3 | 2 | 3 | 2, h, w); c3d_var only with dim_var
    // backward: upstream gradients (each may be NULL = zero) and the three results
    const float *g_noc, *g_ls, *g_c3d, *g_c3d_var, *g_lspx, *g_dims, *g_dims_var;
    void *grad_all_pred;                       // (n, 2 Cn 5, h, w) in all_pred's dtype: every element written
    float *grad_dim, *grad_dim_var;            // (n, 3); grad_dim_var only with dim_var
};

// d of decode_logstd for one object: torch's clamp(min) (a NaN distance stays NaN), or sd itself without distances (q's divisor is then K2's sd_sq)
__device__ __forceinline__ float train_distance(const DecodeTrainArgs &t, int b) {
    if (!t.distances) return t.sdf;
    const float x = t.distances[b];
    return x < t.dist_min ? t.dist_min : x;
}

__global__ void __launch_bounds__(256) noc_decode_train_kernel(const DecodeTrainArgs t) {
#pragma clang fp contract(off)
    const DecodeArgs &a = t.d;
    const int hw = a.h * a.w;
    const int bpo = (hw + 255) >> 8;                   // blocks per object; 1-D grid: n * bpo <= 2^31 - 1
    const int b = blockIdx.x / bpo;
    const int p = (blockIdx.x - b * bpo) * 256 + threadIdx.x;
    DecodeObj o;
    decode_object<false>(a, b, o);
    if (p == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.dims[b * 3 + k] = o.dm[k];
            if (a.has_var) a.dims_var[b * 3 + k] = o.dv[k];
        }
    }
    if (p >= hw) return;
    const float d = train_distance(t, b);
    const float dd = d * d;
    float xv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float noc = pred_at(a, o.base + (long long)(o.ch_noc + k) * hw + p);
        const float part = noc * o.ns[k] + o.nm[k];
        xv[k] = o.dv[k] * (part * part);
        const long long i = ((long long)b * 3 + k) * hw + p;
        t.noc[i] = noc;
        a.c3d[i] = part * o.dm[k];
        if (a.has_var) t.c3d_var[i] = xv[k];
    }
    const float v2[2] = { 0.5f * (xv[0] + xv[2]), xv[1] };
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float ls = pred_at(a, o.base + (long long)(o.ch_ls + k) * hw + p);
        float lspx;
        if (a.has_var) lspx = 0.5f * mr_logf((v2[k] * a.k_epi + mr_expf(2.0f * ls) * a.k_sd2) / dd);
        else lspx = ls + mr_logf(t.sdf / d);
        const long long i = ((long long)b * 2 + k) * hw + p;
        t.ls[i] = ls;
        t.lspx[i] = lspx;
    }
}

// one element of grad_all_pred, in all_pred's dtype (round to nearest even, as torch casts)
__device__ __forceinline__ void grad_pred_store(const DecodeTrainArgs &t, long long i, float v) {
    if (t.d.pred_dtype == MR_F32) { ((float *)t.grad_all_pred)[i] = v; return; }
    if (t.d.pred_dtype == MR_F16) { ((__half *)t.grad_all_pred)[i] = __float2half_rn(v); return; }
    const unsigned u = __float_as_uint(v);
    ((unsigned short *)t.grad_all_pred)[i] = (v != v) ? (unsigned short)0x7fc0 : (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);      // bfloat16
}

// Backward: one workgroup per object, threads stride over the pixels.  The forward is recomputed in registers from all_pred (the same mr_expf):
// nothing is saved but the inputs.  With t = d^2 q of the forward (d itself only adds the constant -log d to the pixel log-std: the backward
// never reads the distances):
//   g_ls_j   = G_ls_j + G_px_j exp(2 ls_j) sd^2 / t_j          (without variance: G_ls_j + G_px_j)
//   g_v2d_j  = G_px_j 0.5 k_epi / t_j
//   g_var_k  = G_var_k + (0.5 g_v2d_0 for k = 0, 2; g_v2d_1 for k = 1)
//   g_part_k = G_c3d_k dims_k + 2 g_var_k dims_var_k part_k,      g_noc_k = G_noc_k + g_part_k s_k
// Every one of the object's 2 Cn 5 channels of grad_all_pred is WRITTEN (the five selected ones with the values, the others with 0): no memset
// launch, no atomics.  The six per-object sums  sum_p G_c3d_k part_k  and  sum_p g_var_k part_k^2  are accumulated per thread in fp64, reduced
// within the wave and then over the four waves through LDS in a fixed order; thread 0 writes grad_dim and grad_dim_var.  Bitwise reproducible.
__global__ void __launch_bounds__(256) noc_decode_train_backward_kernel(const DecodeTrainArgs t) {
#pragma clang fp contract(off)
    __shared__ double red[4][6];
    const DecodeArgs &a = t.d;
    const int hw = a.h * a.w;
    const int b = blockIdx.x;
    DecodeObj o;
    decode_object<false>(a, b, o);
    const int nch = 2 * (a.agnostic ? 1 : a.C) * 5;
    for (int ch = 0; ch < nch; ++ch) {
        if ((unsigned)(ch - o.ch_noc) < 3u || (unsigned)(ch - o.ch_ls) < 2u) continue;
        for (int p = threadIdx.x; p < hw; p += 256) grad_pred_store(t, o.base + (long long)ch * hw + p, 0.0f);
    }
    const bool px_var = a.has_var && t.g_lspx;
    double acc[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int p = threadIdx.x; p < hw; p += 256) {
        float part[3], xv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float noc = pred_at(a, o.base + (long long)(o.ch_noc + k) * hw + p);
            part[k] = noc * o.ns[k] + o.nm[k];
            xv[k] = o.dv[k] * (part[k] * part[k]);
        }
        const float v2[2] = { 0.5f * (xv[0] + xv[2]), xv[1] };
        float g_v2d[2] = { 0.0f, 0.0f };
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long i = ((long long)b * 2 + j) * hw + p;
            const float G_ls = t.g_ls ? t.g_ls[i] : 0.0f;
            const float G_px = t.g_lspx ? t.g_lspx[i] : 0.0f;
            float g_ls = G_ls + G_px;
            if (px_var) {
                const float ls = pred_at(a, o.base + (long long)(o.ch_ls + j) * hw + p);
                const float e = mr_expf(2.0f * ls) * a.k_sd2;
                const float tt = v2[j] * a.k_epi + e;
                g_ls = G_ls + G_px * e / tt;
                g_v2d[j] = G_px * (0.5f * a.k_epi) / tt;
            }
            grad_pred_store(t, o.base + (long long)(o.ch_ls + j) * hw + p, g_ls);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long long i = ((long long)b * 3 + k) * hw + p;
            const float G_c3d = t.g_c3d ? t.g_c3d[i] : 0.0f;
            const float G_noc = t.g_noc ? t.g_noc[i] : 0.0f;
            float g_var = 0.0f;
            if (a.has_var) g_var = (t.g_c3d_var ? t.g_c3d_var[i] : 0.0f) + (k == 1 ? g_v2d[1] : 0.5f * g_v2d[0]);
            const float g_part = G_c3d * o.dm[k] + 2.0f * g_var * o.dv[k] * part[k];
            grad_pred_store(t, o.base + (long long)(o.ch_noc + k) * hw + p, G_noc + g_part * o.ns[k]);
            acc[k] += (double)G_c3d * (double)part[k];
            acc[3 + k] += (double)g_var * ((double)part[k] * (double)part[k]);
        }
    }
    wave_allreduce<6>(acc);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int lab = (int)a.labels[b];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sd = a.dim_stds[lab * 3 + k];
        const double s_dims = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        const double s_var = ((red[0][3 + k] + red[1][3 + k]) + red[2][3 + k]) + red[3][3 + k];
        t.grad_dim[b * 3 + k] = (float)(((t.g_dims ? (double)t.g_dims[b * 3 + k] : 0.0) + s_dims) * (double)sd);
        if (a.has_var) t.grad_dim_var[b * 3 + k] = (float)(((t.g_dims_var ? (double)t.g_dims_var[b * 3 + k] : 0.0) + s_var) * (double)(sd * sd));
    }
}
