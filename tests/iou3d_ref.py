"""numpy restatement of the height / volume composition of the aligned 3-D IoU (bev_to_box3d_overlaps_aligned_torch,
bbox3d_iou_calculator.py:132-163), in float32 and in the kernel's operation order (csrc/iou3d_kernel.inc).  Fed the BEV
intersection areas, it gives what the kernel must return bit for bit.  Used by the CPU and the GPU tests of DESIGN.md §11."""
import numpy as np

F = np.float32


def compose(boxes, qboxes, rinc, criterion, z_center, z_axis=1, rule='reference'):
    """boxes, qboxes (n, 7) [x, y, z, l, h, w, ry]; rinc (n,); criterion and z_center scalars or (n,) arrays.
    rule 'reference': the lower edge of the overlap is min(tops) (torch.min at :145); 'geometric': max(tops) (numpy function, :84)."""
    b, q, r = np.asarray(boxes, F), np.asarray(qboxes, F), np.asarray(rinc, F)
    n = len(b)
    crit = np.broadcast_to(np.asarray(criterion), (n,))
    zc64 = np.broadcast_to(np.asarray(z_center, np.float32).astype(np.float64), (n,))
    up, zc = (1.0 - zc64).astype(F), zc64.astype(F)
    with np.errstate(all='ignore'):
        min_z = np.minimum(b[:, z_axis] + b[:, z_axis + 3] * up, q[:, z_axis] + q[:, z_axis + 3] * up)
        bt, qt = b[:, z_axis] - b[:, z_axis + 3] * zc, q[:, z_axis] - q[:, z_axis + 3] * zc
        max_z = np.minimum(bt, qt) if rule == 'reference' else np.maximum(bt, qt)
        iw = np.maximum(min_z - max_z, F(0))
        v1 = b[:, 3] * b[:, 4] * b[:, 5]
        v2 = q[:, 3] * q[:, 4] * q[:, 5]
        inc = iw * r
        ua = np.select([crit == -1, crit == 0, crit == 1], [v1 + v2 - inc, v1, v2], F(1))
        iou = inc / np.maximum(ua, F(1e-6))
        return np.minimum(np.maximum(iou, F(0)), F(1)).astype(F)
