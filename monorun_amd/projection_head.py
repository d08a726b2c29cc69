"""The NOC head's projection head and its loss (N6): ``UncertProjectionHead`` and ``DistanceInvarProjErrorCoder`` of the
reference (monorun/models/roi_heads/bbox_3d_heads/reprojection_heads/uncert_projection_head.py,
monorun/core/bbox_3d/proj_error_coder/distance_invar_proj_error_coder.py), without mmdet.

In training, the RoI head projects the predicted object coordinates with the ground-truth pose (``forward``), encodes the pixel error
against the RoI grid with the ground-truth distance and feeds it, with the predicted ``proj_logstd``, to ``loss_proj``
(``RobustKLLoss``; monorun_roi_head.py:374-394).  In the shipped configs with ``loss_noc=None`` this is the only loss of the NOC head.

Hot path: ``forward`` on CUDA tensors with an (n, 4) pose runs one HIP launch (``mr_uncert_projection``) and its backward one
(``mr_uncert_projection_backward``); ``RobustKLLoss`` runs its own two plus one (monorun_amd/losses.py).  The encode between them
stays in torch, so ``coords_2d_roi`` and ``distances`` get the gradients the reference's graph gives them.  Other inputs (CPU tensors,
leading pose dimensions, ground truth that requires grad) run :func:`uncert_projection`, the torch restatement.
"""
import torch
import torch.nn as nn

from .losses import build_loss


class DistanceInvarProjErrorCoder:
    """Scales pixel errors and log-stds by distance / (ref_length * ref_focal_y * target_std), so that the encoded error of an
    object does not depend on how far away it is.  Differentiable torch; the reference's defaults (``target_std`` 0.25; the
    shipped configs pass 0.15)."""

    def __init__(self, ref_length=1.6, ref_focal_y=722, target_std=0.25, distance_min=0.1, epistemic_std_gain=1.0):
        self.scaling_denomitor = ref_length * ref_focal_y * target_std     # the reference's attribute name
        self.ref_focal_y = ref_focal_y
        self.distance_min = distance_min
        self.epistemic_std_gain = epistemic_std_gain

    def encode(self, coords_2d_diff_std, distance):
        """(N, C, H, W) pixel error or std, (N, 1) distance -> encoded."""
        return coords_2d_diff_std * (distance[..., None, None] / self.scaling_denomitor)

    def decode(self, proj_error_std, distance):
        return proj_error_std * (self.scaling_denomitor / distance[..., None, None].clamp(min=self.distance_min))

    def decode_logstd(self, proj_logstd, coords_3d_var, distance):
        """Pixel log-std from the encoded one; with ``coords_3d_var`` (N, 3, H, W) the epistemic variance of the coordinates is
        added.  ``distance`` (N, 1), or None: the reference distance, i.e. the identity scale."""
        sd = self.scaling_denomitor
        if distance is None:
            dist = proj_logstd.new_tensor([sd])
        else:
            dist = distance[..., None, None].clamp(min=self.distance_min)
        if coords_3d_var is None:
            return proj_logstd + torch.log(sd / dist)
        var_2d = torch.stack((0.5 * (coords_3d_var[:, 0] + coords_3d_var[:, 2]), coords_3d_var[:, 1]), dim=1)
        var_2d = (var_2d * (self.ref_focal_y * self.epistemic_std_gain) ** 2 + (2 * proj_logstd).exp() * sd ** 2) / dist.square()
        return 0.5 * torch.log(var_2d)

    def cov_correction(self, cov, distance):
        return cov * (self.scaling_denomitor / distance).square().view(-1, 1, 1)


PROJ_ERROR_CODERS = {'DistanceInvarProjErrorCoder': DistanceInvarProjErrorCoder}


def build_proj_error_coder(cfg):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ not in PROJ_ERROR_CODERS:
        raise ValueError(f'unknown projection error coder {typ!r}')
    return PROJ_ERROR_CODERS[typ](**cfg)


def uncert_projection(coords_3d, pose, cam_intrinsic, img_shapes, z_min=0.5, allowed_border=200):
    """Torch restatement of the projection: coords_3d (n, 3, h, w), pose (..., n, 4) [x, y, z, yaw], cam_intrinsic (n, 3, 3),
    img_shapes (n, 2) [H, W] -> (..., n, 2, h, w) pixel coordinates, z clamped to ``z_min`` and the result clamped to the image
    widened by ``allowed_border``."""
    n, _, h, w = coords_3d.size()
    yaw = pose[..., 3]
    s, c = torch.sin(yaw), torch.cos(yaw)
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    rot = torch.stack((c, zero, s, zero, one, zero, -s, zero, c), dim=-1).reshape(pose.shape[:-1] + (3, 3))
    p_r = cam_intrinsic @ rot
    p_t = cam_intrinsic @ pose[..., :3, None]
    proj = (p_r @ coords_3d.reshape(n, 3, h * w) + p_t).reshape(pose.shape[:-1] + (3, h, w))
    uv, z = proj.split([2, 1], dim=-3)
    uv = (uv / z.clamp(min=z_min)).clamp(min=-allowed_border)
    return torch.min(uv, img_shapes[:, [1, 0], None, None] + allowed_border)


class _ProjectionFunction(torch.autograd.Function):
    """``mr_uncert_projection`` forward, ``mr_uncert_projection_backward`` for the gradient to coords_3d (the other inputs are
    ground truth).  coords_3d, K and img_shapes arrive as contiguous fp32; pose as fp32 rows with unit column stride."""

    @staticmethod
    def forward(ctx, coords_3d, pose, cam_intrinsic, img_shapes, z_min, allowed_border):
        from . import _lib
        n, _, h, w = coords_3d.shape
        out = coords_3d.new_empty((n, 2, h, w))
        if n:
            dev = coords_3d.device
            with torch.cuda.device(dev):
                _lib.call('mr_uncert_projection', coords_3d=coords_3d.data_ptr(), pose=pose.data_ptr(), pose_row_stride=pose.stride(0),
                          cam_intrinsic=cam_intrinsic.data_ptr(), img_shapes=img_shapes.data_ptr(), n=n, hw=h * w, z_min=z_min,
                          allowed_border=allowed_border, coords_2d=out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(coords_3d, pose, cam_intrinsic, img_shapes)
        ctx.args = (z_min, allowed_border)
        return out

    @staticmethod
    def backward(ctx, grad):
        from . import _lib
        coords_3d, pose, cam_intrinsic, img_shapes = ctx.saved_tensors
        z_min, allowed_border = ctx.args
        n, _, h, w = coords_3d.shape
        grad_3d = torch.empty_like(coords_3d)
        if n:
            grad = grad.to(torch.float32).contiguous()
            dev = coords_3d.device
            with torch.cuda.device(dev):
                _lib.call('mr_uncert_projection_backward', coords_3d=coords_3d.data_ptr(), pose=pose.data_ptr(), pose_row_stride=pose.stride(0),
                          cam_intrinsic=cam_intrinsic.data_ptr(), img_shapes=img_shapes.data_ptr(), n=n, hw=h * w, z_min=z_min,
                          allowed_border=allowed_border, grad_coords_2d=grad.data_ptr(), grad_coords_3d=grad_3d.data_ptr(),
                          stream=torch.cuda.current_stream(dev).cuda_stream)
        return grad_3d, None, None, None, None, None


def _projection_hip_ok(coords_3d, pose, cam_intrinsic, img_shapes):
    ts = (coords_3d, pose, cam_intrinsic, img_shapes)
    if not all(isinstance(t, torch.Tensor) and t.is_floating_point() for t in ts):
        return False
    dev = coords_3d.device
    if dev.type != 'cuda' or any(t.device != dev for t in ts):
        return False
    if coords_3d.dim() != 4 or coords_3d.size(1) != 3 or coords_3d.size(2) * coords_3d.size(3) == 0:
        return False
    n = coords_3d.size(0)
    if pose.shape != (n, 4) or cam_intrinsic.shape != (n, 3, 3) or img_shapes.shape != (n, 2):
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in ts[1:]))


def _pose_rows(pose):
    """fp32 (n, 4) rows the kernel reads in place: unit column stride, any row stride >= 4 (e.g. pos_bboxes_3d[:, 3:7])"""
    pose = pose.detach().to(torch.float32)
    return pose if pose.stride(1) == 1 and pose.stride(0) >= 4 else pose.contiguous()


class UncertProjectionHead(nn.Module):
    """The reference's projection head: same constructor defaults, attributes, methods and ``state_dict`` keys
    (``loss_proj.mean_inv_std``).  ``get_properties`` takes any sampling results with ``pos_inds`` and ``pos_assigned_gt_inds``
    and ``img_metas`` dicts."""

    def __init__(self,
                 loss_proj=dict(type='RobustKLLoss', loss_weight=1.0, momentum=0.1),
                 z_min=0.5,
                 allowed_border=200,
                 proj_error_coder=dict(type='DistanceInvarProjErrorCoder', ref_length=1.6, ref_focal_y=722, target_std=0.15),
                 distance_mode='range'):
        super().__init__()
        self.loss_proj = build_loss(loss_proj) if loss_proj is not None else None
        self.z_min = z_min
        self.allowed_border = allowed_border
        self.proj_error_coder = build_proj_error_coder(proj_error_coder)
        self.fp16_enabled = False
        if distance_mode not in ('z-depth', 'range'):
            raise ValueError(f'distance_mode must be "z-depth" or "range", not {distance_mode!r}')
        self.distance_mode = distance_mode
        self.train_std_of_encoded_error = True

    def forward(self, coords_3d, pose, cam_intrinsic, img_shapes):
        """
        Args:
            coords_3d (Tensor): (n, 3, h, w) object coordinates
            pose (Tensor): (..., n, 4) [x, y, z, yaw]
            cam_intrinsic (Tensor): (n, 3, 3)
            img_shapes (Tensor): (n, 2) [H, W]

        Returns:
            Tensor: (..., n, 2, h, w) projected pixel coordinates
        """
        if _projection_hip_ok(coords_3d, pose, cam_intrinsic, img_shapes):
            out = _ProjectionFunction.apply(coords_3d.to(torch.float32).contiguous(), _pose_rows(pose),
                                            cam_intrinsic.detach().to(torch.float32).contiguous(),
                                            img_shapes.detach().to(torch.float32).contiguous(), float(self.z_min), float(self.allowed_border))
            return out.to(coords_3d.dtype)
        return uncert_projection(coords_3d, pose, cam_intrinsic, img_shapes, self.z_min, self.allowed_border)

    def get_properties(self, sampling_results, cam_intrinsic, gt_bboxes_3d, img_metas):
        """Per positive RoI: camera matrix (Npos, 3, 3), assigned ground-truth box (Npos, 7) [l, h, w, x, y, z, yaw], distance
        (Npos, 1) and image shape (Npos, 2) [H, W]."""
        img_shapes, pos_k = [], []
        for img_meta, k, res in zip(img_metas, cam_intrinsic, sampling_results):
            npos = len(res.pos_inds)
            img_shapes += [list(img_meta['img_shape'][:2])] * npos
            pos_k += [k] * npos
        if img_shapes:
            img_shapes = cam_intrinsic[0].new_tensor(img_shapes)
            pos_k = torch.stack(pos_k, dim=0)
        else:
            img_shapes = cam_intrinsic[0].new_zeros((0, 2))
            pos_k = cam_intrinsic[0].new_zeros((0, 3, 3))
        pos_bboxes_3d = torch.cat([gt[res.pos_assigned_gt_inds] for gt, res in zip(gt_bboxes_3d, sampling_results)], dim=0)
        if self.distance_mode == 'z-depth':
            distances = pos_bboxes_3d[:, 5:6]
        else:
            distances = torch.norm(pos_bboxes_3d[:, 3:6], p=2, dim=1, keepdim=True)
        return pos_k, pos_bboxes_3d, distances, img_shapes

    def get_distance(self, t_vec):
        if self.distance_mode == 'z-depth':
            return t_vec[:, 2]
        return torch.norm(t_vec, p=2, dim=1)

    def loss(self, coords_2d_proj, coords_2d_norm_logstd, coords_2d_roi, distances):
        if self.loss_proj is None:
            return dict()
        proj_error = self.proj_error_coder.encode(coords_2d_proj - coords_2d_roi, distances)
        if proj_error.size(0) == 0:
            # no positive RoI: a zero that keeps the graph, and the loss (with its running buffer) is not called
            loss_proj = proj_error.sum() + coords_2d_norm_logstd.sum()
        else:
            loss_proj = self.loss_proj(proj_error, 0, logstd=coords_2d_norm_logstd)
        return dict(loss_proj=loss_proj)

    def loss_empty(self, device):
        if self.loss_proj is None:
            return dict()
        return dict(loss_proj=torch.zeros(1, device=device, dtype=torch.float32))
