// nms_order.inc — the order in which the rotated-BEV NMS visits a group's boxes, and the padded bitonic network that produces it.
// No HIP dependency: nms_bev_kernel (consumers_kernel.inc) compiles it with MR_NMS_FN = __device__ __forceinline__, the oracle's C
// library (oracle/pnp_oracle.c, orc_nms_order) with MR_NMS_FN = static inline, so the host can run the very network the kernel runs.
//
// The order is total on (score, index):
//   1. non-NaN scores before NaN scores;
//   2. among non-NaN scores, descending score (+inf first, -inf last);
//   3. equal scores by ascending index;
//   4. NaN scores among themselves by ascending index;
//   5. padding (index MR_NMS_PAD_INDEX) after everything.
// It deviates from torch.sort(descending=True), which puts NaN first.
#ifndef MR_NMS_FN
#error "define MR_NMS_FN (the function qualifiers) before including nms_order.inc"
#endif

#define MR_NMS_PAD_INDEX 0x7fffffff

// "a before b" in the final order.  Two padding entries are equal: neither is before the other.
MR_NMS_FN int mr_nms_before(float ka, int ia, float kb, int ib) {
    const int ca = (ia == MR_NMS_PAD_INDEX) ? 2 : (ka != ka) ? 1 : 0;   // class: finite or infinite score, NaN score, padding
    const int cb = (ib == MR_NMS_PAD_INDEX) ? 2 : (kb != kb) ? 1 : 0;
    if (ca != cb) return ca < cb;
    if (ca == 0 && ka != kb) return ka > kb;
    return ia < ib;
}

// The network's size for n entries: the next power of two.
MR_NMS_FN int mr_nms_padded(int n) {
    int np2 = 1;
    while (np2 < n) np2 <<= 1;
    return np2;
}

// Entry i of the padded arrays before the sort.
MR_NMS_FN void mr_nms_fill(float *key, int *idx, int i, int n, const float *scores) {
    key[i] = (i < n) ? scores[i] : 0.0f;
    idx[i] = (i < n) ? i : MR_NMS_PAD_INDEX;
}

// Position i's part of the network's step (k, j): k = 2, 4, .., np2 outer, j = k / 2, k / 4, .., 1 inner; every position of a step may
// run concurrently, and a barrier separates the steps.  The lower position of each pair (i, i ^ j) does the compare-exchange.
MR_NMS_FN void mr_nms_step(float *key, int *idx, int i, int j, int k) {
    const int l = i ^ j;
    if (l > i) {
        const float ki = key[i], kl = key[l];
        const int ii = idx[i], il = idx[l];
        const int i_first = mr_nms_before(ki, ii, kl, il);
        const int up = (i & k) == 0;
        if (up ? !i_first : i_first) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
    }
}
