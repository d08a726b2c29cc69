// iou3d_kernel.inc — N5 (DESIGN.md §11): aligned rotated 3-D IoU, the IoU the pose head's training loss reports and the score head
// learns (uncert_prop_pnp_optimizer.py:118-124 -> bbox3d_overlaps_aligned_torch, bbox3d_iou_calculator.py:166-192).
//
// The reference makes two steps of it: a numba-CUDA launch for the BEV intersection area (rotate_iou_kernel_eval_aligned,
// rotate_iou_calculator.py:68-92, devRotateIoUEval(box, qbox, criterion=2)) and a chain of torch element-wise ops for the
// height and volume composition (bev_to_box3d_overlaps_aligned_torch, bbox3d_iou_calculator.py:132-163).  Here one thread does
// both for one pair (box i, query box i).  No LDS, no atomics, no scratch; every output is one ordinary global store.
//
// Rows are 7 fp32 values [x, y, z, l, h, w, ry] at a row stride (in elements, >= 7); z_axis names the height axis (1 for KITTI
// camera boxes), z_center the height centre (1.0: the coordinate is the bottom of the box, y pointing down).
//
// BEV area: eval_rotated_intersection (kitti_eval_kernel.inc), the corner convention of rbbox_to_corners, inputs rounded to fp32,
// result rounded to fp32 — the value the numba kernel stores.  The box is the first argument, as in the aligned numba kernel.  The
// routine's one rule (edge_inside_area_t): coincident edges of the same direction are counted once, coincident edges of opposite direction
// never, decided unfused — identical boxes give their area, boxes that only touch give 0.  The numba kernel is degenerate on identical
// boxes (1/3 or 0 of the area).
//
// Height rules (flags):
//   default, "reference":      max_z = min(box_top, qbox_top) — what bev_to_box3d_overlaps_aligned_torch computes (:145, torch.min),
//                              the IoU every MonoRUn score head was trained against.  It ignores vertical misalignment in one direction.
//   MR_IOU3D_GEOMETRIC_HEIGHT: max_z = max(box_top, qbox_top) — the geometric overlap, as the numpy sibling (:84) and the N x K form (:28).
// Composition in fp32, operation for operation (no contraction):
//   iw = clamp(min_z - max_z, 0); v1 = (l*h)*w; v2 likewise; inc = iw * rinc; ua = v1 + v2 - inc | v1 | v2 | 1 (criterion -1 | 0 | 1 | 2);
//   iou = clamp(inc / clamp(ua, 1e-6), 0, 1).  min / max / clamp propagate NaN, as torch's do (nan_min ... clamp_hi, kitti_eval_kernel.inc).

__global__ void __launch_bounds__(256) bbox3d_overlaps_aligned_kernel(const float *__restrict__ boxes, long long boxes_stride,
                                                                      const float *__restrict__ qboxes, long long qboxes_stride, int n,
                                                                      int criterion, int z_axis, float z_center, int geometric,
                                                                      float *__restrict__ iou, float *__restrict__ rinc_out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *b = boxes + (long long)i * boxes_stride, *q = qboxes + (long long)i * qboxes_stride;
    // BEV box = the row without the height coordinate and its size: [cx, cy, dx, dy, angle].  Runtime column offsets are read
    // straight from memory (no private array indexed at run time, hence no scratch).
    const int a0 = z_axis == 0 ? 1 : 0, a1 = z_axis == 2 ? 1 : 2;
    const double bb[5] = { (double)b[a0], (double)b[a1], (double)b[a0 + 3], (double)b[a1 + 3], (double)b[6] };
    const double qb[5] = { (double)q[a0], (double)q[a1], (double)q[a0 + 3], (double)q[a1 + 3], (double)q[6] };
    const float rinc = (float)eval_rotated_intersection(bb, qb);
    // height and volume composition (bbox3d_iou_calculator.py:140-163)
    const float up = (float)(1.0 - (double)z_center);     // the Python scalar (1 - z_center), rounded to the tensor's fp32
    const float bz = b[z_axis], bh = b[z_axis + 3], qz = q[z_axis], qh = q[z_axis + 3];
    const float min_z = nan_min(bz + bh * up, qz + qh * up);
    const float bt = bz - bh * z_center, qt = qz - qh * z_center;
    const float max_z = geometric ? nan_max(bt, qt) : nan_min(bt, qt);
    const float iw = clamp_lo(min_z - max_z, 0.0f);
    const float v1 = b[3] * b[4] * b[5], v2 = q[3] * q[4] * q[5];
    const float inc = iw * rinc;
    float ua;
    if (criterion == -1) ua = v1 + v2 - inc;
    else if (criterion == 0) ua = v1;
    else if (criterion == 1) ua = v2;
    else ua = 1.0f;
    const float r = inc / clamp_lo(ua, 1e-6f);
    iou[i] = clamp_hi(clamp_lo(r, 0.0f), 1.0f);
    if (rinc_out) rinc_out[i] = rinc;
}
