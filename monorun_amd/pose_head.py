"""Host-side mirror of the glue either side of the PnP on the hot path (forward / inference only).

  * ``noc_decode``  — K2, one HIP kernel for R9-R12 + the istd / RANSAC-threshold part of R8
    (fcn_noc_decoder.py:225-267, multiclass_norm_dim_coder.py:28-36, noc_coder.py:50-73,
    distance_invar_proj_error_coder.py:39-60, uncert_prop_pnp_optimizer.py:73,86-88,
    roi_align(coord_2d) at monorun_roi_head.py:521-523)
  * ``UncertPropPnPOptimizer`` — same constructor / ``forward`` / ``get_targets`` / ``loss`` contract as
    the reference's monorun/models/roi_heads/bbox_3d_heads/optimizers/uncert_prop_pnp_optimizer.py:12-159
    (the loss's 3-D IoU is the HIP kernel of ``iou3d``, its losses are torch: ``losses``)
  * ``cov_correction`` — R13 (distance_invar_proj_error_coder.py:62-63 with the 'range' distance of
    uncert_projection_head.py:104-109), applied at monorun_roi_head.py:530-534
  * ``pnp_from_head`` / ``pose_from_head`` — the whole post-NOC-head tail in ONE launch (K2 fused into the PnP kernel's
    load stage; the decoded maps never touch HBM), or two launches with ``fused=False``
"""
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .iou3d import bbox3d_overlaps_aligned
from .losses import build_loss
from .ops import build_pnp

# coder constants of the shipped configs (configs/kitti_multiclass.py / kitti_car.py; coder defaults)
NOC_MEANS = (-0.1, -0.5, 0.0)
NOC_STDS = (0.35, 0.23, 0.34)
DIM_MEANS = ((3.89, 1.53, 1.62), (0.82, 1.78, 0.63), (1.77, 1.72, 0.57))
DIM_STDS = ((0.44, 0.14, 0.11), (0.25, 0.13, 0.12), (0.15, 0.10, 0.14))


_CONST_CACHE = {}
_CONST_BY_ID = {}


def _const(values, dev):
    """Small constant tensors (coder means/stds, clip ranges) live on the device once per (device, value).  The same
    Python object (the module-level defaults, a config tuple) is recognised by identity without being re-hashed."""
    ik = (id(values), dev)
    hit = _CONST_BY_ID.get(ik)
    if hit is not None and hit[0] is values:
        return hit[1]
    arr = np.asarray(values, np.float32)
    key = (str(dev), arr.tobytes(), arr.shape)
    t = _CONST_CACHE.get(key)
    if t is None:
        t = torch.tensor(arr, device=dev).contiguous()
        _CONST_CACHE[key] = t
    if not isinstance(values, np.ndarray) or not values.flags.writeable:      # a mutable array may change under the same id
        if len(_CONST_BY_ID) > 256:
            _CONST_BY_ID.clear()
        _CONST_BY_ID[ik] = (values, t)
    return t


_RANGE_CACHE = {}


def _hw_rows(img_shapes):
    """(n, 2) [H, W] rows from what the pipeline passes: a (H, W) or mmdet (H, W, 3) tuple of ONE image
    (img_meta['img_shape']; the reference indexes only [:, 0] and [:, 1], uncert_prop_pnp_optimizer.py:75-80), or an
    (n, 2) / (n, 3) array or tensor of per-image rows."""
    if torch.is_tensor(img_shapes):
        sh = img_shapes if img_shapes.dim() == 2 else img_shapes.reshape(1, -1)
    else:
        sh = np.asarray(img_shapes, np.float32)
        sh = sh if sh.ndim == 2 else sh.reshape(1, -1)
    assert sh.shape[1] in (2, 3), f'img_shape must be (H, W), (H, W, C) or rows of them, got shape {tuple(sh.shape)}'
    return sh[:, :2]


def _clip_ranges(img_shapes, allowed_border, dev):
    """u_range = [-border, W + border], v_range = [-border, H + border] (uncert_prop_pnp_optimizer.py:75-80)."""
    img_shapes = _hw_rows(img_shapes)
    if torch.is_tensor(img_shapes) and img_shapes.device.type == 'cuda':
        sh = img_shapes.to(torch.float32).reshape(-1, 2)
        ur = sh.new_full((sh.size(0), 2), -float(allowed_border)); vr = ur.clone()
        ur[:, 1] = sh[:, 1] + allowed_border; vr[:, 1] = sh[:, 0] + allowed_border
        return ur, vr
    sh = np.asarray(img_shapes.cpu() if torch.is_tensor(img_shapes) else img_shapes, np.float32).reshape(-1, 2)
    key = (sh.tobytes(), float(allowed_border), dev)
    hit = _RANGE_CACHE.get(key)
    if hit is None:
        ur = np.stack([np.full(len(sh), -float(allowed_border), np.float32), sh[:, 1] + allowed_border], 1)
        vr = np.stack([np.full(len(sh), -float(allowed_border), np.float32), sh[:, 0] + allowed_border], 1)
        if len(_RANGE_CACHE) > 256:
            _RANGE_CACHE.clear()
        hit = _RANGE_CACHE[key] = (torch.tensor(ur, device=dev), torch.tensor(vr, device=dev))
    return hit


_PRED_DTYPES = {torch.float32: _lib.MR_F32, torch.float16: _lib.MR_F16, torch.bfloat16: _lib.MR_BF16}


def _head_output(all_pred, dev):
    """The NOC head's output as the kernels take it: fp32, fp16 or bf16 (autocast) is read as is, anything else -> fp32."""
    x = all_pred.detach()
    if x.dtype not in _PRED_DTYPES or x.device != dev:
        x = x.to(device=dev, dtype=x.dtype if x.dtype in _PRED_DTYPES else torch.float32)
    return (x if x.is_contiguous() else x.contiguous()), _PRED_DTYPES[x.dtype]


def _coord_map(coord_2d, dev):
    """The optional coord_2d map as the kernels read it: a contiguous fp32 (2,H,W) tensor on `dev` (the input itself when it
    already is one, otherwise a converted COPY — whoever keeps the pointer beyond one launch must keep this tensor), or None."""
    if coord_2d is None:
        return None
    m = coord_2d.detach().to(device=dev, dtype=torch.float32)
    m = m[0] if m.dim() == 4 else m
    assert m.dim() == 3 and m.shape[0] == 2, 'coord_2d must be (1,2,H,W) or (2,H,W) — one image per call'
    return m.contiguous()


def _coord_map_args(m):
    """The coord_2d_map / map_h / map_w arguments of the kernels for `_coord_map`'s tensor (None: no map).  For ONE launch that is
    enqueued right away a converted copy may be released at once (the caching allocator is stream-ordered); a prepared launch must
    hold the tensor."""
    return dict(coord_2d_map=_lib.ptr(m), map_h=int(m.shape[1]) if m is not None else 0, map_w=int(m.shape[2]) if m is not None else 0)


def gen_coord_2d(h, w, pad_to=32, flip=False, scale=None, device=None):
    """The image's coordinate map as the reference's data pipeline hands it to the RoI head — ``(1, 2, Hp, Wp)`` float32, channel 0 =
    u (column index), channel 1 = v (row index) of the ORIGINAL image:

      * ``LoadAnnotations3D._gen_coord_2d`` (/root/reference/monorun/datasets/pipelines/loading.py:67-78): ``np.mgrid[:h, :w]``, [u, v];
      * ``flip``: RandomFlip3D's horizontal ``mmcv.imflip`` of the dense field (transforms.py:36-52): column x' holds u = w - 1 - x';
      * ``pad_to``: Pad3D's ``mmcv.impad(..., padding_mode='edge')`` to the next multiple of ``size_divisor`` (transforms.py:55-74;
        configs/kitti_car.py:220,238): rows / columns beyond the image REPLICATE the last row / column (0 = no padding).
      These three are index operations and are pinned by fixture G9 (generated by calling the reference's function).
      * ``scale`` (keep-ratio factor s of Resize3D, transforms.py:12-32; no shipped config uses it): the bilinear branch of
        ``mmcv.imrescale`` for s >= 1 — cv2's half-pixel mapping of a linear ramp, u(x') = clip((x' + 0.5) / s - 0.5, 0, w - 1) —
        applied before flip and padding as the pipeline orders them.  OpenCV is not in this image: unpinned; s < 1 ('area') is refused.

    ``coord_2d=None`` in ``noc_decode`` / ``pose_from_head`` (bin centres written analytically) equals RoIAlign of this map exactly
    where every sampling point of the RoI lies inside [0, w - 1] x [0, h - 1] of an unflipped, unscaled image; RoIs that hug or cross the
    image border, flipped or rescaled images need the map."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError('gen_coord_2d: empty image')
    f32 = dict(dtype=torch.float32, device=device)
    if scale is None or float(scale) == 1.0:
        u = torch.arange(w, **f32)
        v = torch.arange(h, **f32)
    else:
        s = float(scale)
        if s < 1.0:
            raise NotImplementedError("gen_coord_2d: scale < 1 uses cv2's INTER_AREA (mmcv.imrescale), which is not restated")
        ws, hs = int(w * s + 0.5), int(h * s + 0.5)                 # mmcv.rescale_size
        # cv2.resize maps by the per-axis ratio src / dst; float64 arithmetic, float32 storage
        u = ((torch.arange(ws, dtype=torch.float64, device=device) + 0.5) * (w / ws) - 0.5).clamp_(0, w - 1).to(torch.float32)
        v = ((torch.arange(hs, dtype=torch.float64, device=device) + 0.5) * (h / hs) - 0.5).clamp_(0, h - 1).to(torch.float32)
    if flip:
        u = torch.flip(u, dims=[0])
    hh, ww = int(v.numel()), int(u.numel())
    d = int(pad_to) if pad_to else 1
    hp, wp = -(-hh // d) * d, -(-ww // d) * d
    if wp > ww:
        u = torch.cat([u, u[-1:].expand(wp - ww)])
    if hp > hh:
        v = torch.cat([v, v[-1:].expand(hp - hh)])
    out = torch.empty(1, 2, hp, wp, **f32)
    out[0, 0] = u[None, :]
    out[0, 1] = v[:, None]
    return out


def roi_align_avg(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    """mmcv.ops.roi_align(input, rois, output_size, spatial_scale, sampling_ratio, 'avg', aligned) forward
    (``mr_roi_align_avg``).  input (N,C,H,W) f32 on the GPU, rois (K,5) [batch_idx, x1, y1, x2, y2] -> (K,C,oh,ow)."""
    _lib.load()
    dev = input.device
    if dev.type != 'cuda':
        raise RuntimeError('monorun_amd.roi_align_avg runs on an MI355X only (no CPU fallback)')
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else tuple(int(v) for v in output_size)
    x = input.detach().to(torch.float32).contiguous()
    r = rois.detach().to(device=dev, dtype=torch.float32).contiguous()
    N, C, H, W = x.shape
    out = torch.empty(r.shape[0], C, oh, ow, device=dev, dtype=torch.float32)
    if r.shape[0]:
        with torch.cuda.device(dev):
            _lib.call('mr_roi_align_avg', input=x.data_ptr(), rois=r.data_ptr(), K=r.shape[0], C=C, H=H, W=W, out_h=oh, out_w=ow,
                      spatial_scale=float(spatial_scale), sampling_ratio=int(sampling_ratio), aligned=int(bool(aligned)), output=out.data_ptr(),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def _decode_args(all_pred, pred_dtype, labels, flip, dim, dim_var, rois, num_classes, class_agnostic, consts, ref_length, ref_focal_y, target_std,
                 epistemic_std_gain, std_scale, epnp_ransac_thres_ratio):
    """The arguments ``mr_noc_decode_batched`` and ``mr_pnp_from_head_batched`` share (the decode: their first 21), by the header's names.
    consts = the (dim_means, dim_stds, noc_means, noc_stds) device tensors."""
    B, _, h, w = all_pred.shape
    mu, sd, nm, ns = consts
    return dict(all_pred=all_pred.data_ptr(), pred_dtype=pred_dtype, labels=labels.data_ptr(), flip=flip.data_ptr(), dim=dim.data_ptr(),
                dim_var=_lib.ptr(dim_var), rois=rois.data_ptr(), B=B, num_classes=num_classes,
                class_agnostic=int(class_agnostic), h=h, w=w, dim_means=mu.data_ptr(), dim_stds=sd.data_ptr(), noc_means=nm.data_ptr(),
                noc_stds=ns.data_ptr(), proj_scaling_denominator=float(ref_length * ref_focal_y * target_std), ref_focal_y=float(ref_focal_y),
                epistemic_std_gain=float(epistemic_std_gain), std_scale=float(std_scale),
                ransac_thres_ratio=float(epnp_ransac_thres_ratio) if epnp_ransac_thres_ratio is not None else -1.0)


def noc_decode(all_pred, labels, flip, dim, dim_var, rois, num_classes=3, class_agnostic=False,
               dim_means=DIM_MEANS, dim_stds=DIM_STDS, noc_means=NOC_MEANS, noc_stds=NOC_STDS,
               ref_length=1.6, ref_focal_y=722, target_std=0.15, epistemic_std_gain=1.0,
               std_scale=10, epnp_ransac_thres_ratio=0.2, coord_2d=None):
    """Raw NOC-head output -> PnP-boundary maps, on the device, in one kernel.

    all_pred (B, 2*C*5, h, w) f32; labels (B,) int64; flip bool | (B,) bool; dim (B,3); dim_var (B,3)|None;
    rois (B,4) xyxy or (B,5) [batch_idx, x1, y1, x2, y2] (mmdet bbox2roi).
    coord_2d: None (identity pixel grid: bin centres written analytically) or the image's (1,2,H,W)/(2,H,W) coordinate map
    (loading.py:67-78 after resize/flip/pad), sampled with mmcv's exact RoIAlign rule (monorun_roi_head.py:521-523).
    Returns dict(coords_2d (B,2,h,w), coords_2d_istd (B,2,h,w), coords_3d (B,3,h,w), dims (B,3),
                 dims_var (B,3)|None, ransac_thr (B,)|None).
    """
    lib = _lib.load()
    dev = all_pred.device
    if dev.type != 'cuda':
        raise RuntimeError('monorun_amd.noc_decode runs on an MI355X only (no CPU fallback)')
    B, ch, h, w = all_pred.shape
    Cn = 1 if class_agnostic else num_classes
    assert ch == 2 * Cn * 5, f'all_pred has {ch} channels, expected {2 * Cn * 5}'
    f32 = dict(device=dev, dtype=torch.float32)
    ap, ap_dt = _head_output(all_pred, dev)
    lab = labels.detach().to(device=dev, dtype=torch.int64).contiguous()
    fl = _flip_flags(flip, B, dev)
    dm = dim.detach().to(**f32).contiguous()
    dv = dim_var.detach().to(**f32).contiguous() if dim_var is not None else None
    r = rois.detach().to(**f32)
    r = (r[:, 1:5] if r.shape[1] == 5 else r).contiguous()
    mu, sd, nm, ns = _const(dim_means, dev), _const(dim_stds, dev), _const(noc_means, dev), _const(noc_stds, dev)
    assert mu.shape == sd.shape and mu.shape[1] == 3
    c2d = torch.empty(B, 2, h, w, **f32)
    istd = torch.empty(B, 2, h, w, **f32)
    c3d = torch.empty(B, 3, h, w, **f32)
    dims = torch.empty(B, 3, **f32)
    dims_var = torch.empty(B, 3, **f32) if dv is not None else None
    thr = torch.empty(B, **f32) if epnp_ransac_thres_ratio is not None else None
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_noc_decode_batched', **_decode_args(ap, ap_dt, lab, fl, dm, dv, r, num_classes, class_agnostic, (mu, sd, nm, ns),
                      ref_length, ref_focal_y, target_std, epistemic_std_gain, std_scale, epnp_ransac_thres_ratio), coords_2d=c2d.data_ptr(),
                      coords_2d_istd=istd.data_ptr(), coords_3d=c3d.data_ptr(), dims=dims.data_ptr(), dims_var=_lib.ptr(dims_var),
                      ransac_thr=_lib.ptr(thr), **_coord_map_args(_coord_map(coord_2d, dev)), stream=torch.cuda.current_stream(dev).cuda_stream)
    return dict(coords_2d=c2d, coords_2d_istd=istd, coords_3d=c3d, dims=dims, dims_var=dims_var, ransac_thr=thr)


class NocDecodeLaunch:
    """A PREPARED launch of K2 (``mr_noc_decode_batched``) over static input / output tensors: every ctypes argument is built
    once, ``run()`` only enqueues the kernel (the eager ``noc_decode`` allocates six outputs and marshals 30 arguments per call —
    more host time than the ~10 us the kernel takes at B = 1024).  ``out`` has the keys of ``noc_decode``'s result."""

    def __init__(self, all_pred, labels, flip, dim, dim_var, rois, num_classes=3, class_agnostic=False,
                 dim_means=DIM_MEANS, dim_stds=DIM_STDS, noc_means=NOC_MEANS, noc_stds=NOC_STDS,
                 ref_length=1.6, ref_focal_y=722, target_std=0.15, epistemic_std_gain=1.0,
                 std_scale=10, epnp_ransac_thres_ratio=0.2, coord_2d=None):
        self.lib = _lib.load()
        dev = all_pred.device
        if dev.type != 'cuda':
            raise RuntimeError('NocDecodeLaunch runs on an MI355X only (no CPU fallback)')
        self.dev = dev
        B, ch, h, w = all_pred.shape
        Cn = 1 if class_agnostic else num_classes
        assert ch == 2 * Cn * 5, f'all_pred has {ch} channels, expected {2 * Cn * 5}'
        f32 = dict(device=dev, dtype=torch.float32)
        ap, ap_dt = _head_output(all_pred, dev)
        r = rois.detach().to(**f32)
        r = (r[:, 1:5] if r.shape[1] == 5 else r).contiguous()
        cmap = _coord_map(coord_2d, dev)
        self.inputs = dict(all_pred=ap, labels=labels.detach().to(device=dev, dtype=torch.int64).contiguous(), flip=_flip_flags(flip, B, dev).clone(),
                           dim=dim.detach().to(**f32).contiguous(), dim_var=dim_var.detach().to(**f32).contiguous() if dim_var is not None else None,
                           rois=r, coord_2d=cmap)
        i = self.inputs
        mu, sd, nm, ns = _const(dim_means, dev), _const(dim_stds, dev), _const(noc_means, dev), _const(noc_stds, dev)
        self._keep = (mu, sd, nm, ns)
        self.out = dict(coords_2d=torch.empty(B, 2, h, w, **f32), coords_2d_istd=torch.empty(B, 2, h, w, **f32), coords_3d=torch.empty(B, 3, h, w, **f32),
                        dims=torch.empty(B, 3, **f32), dims_var=torch.empty(B, 3, **f32) if dim_var is not None else None,
                        ransac_thr=torch.empty(B, **f32) if epnp_ransac_thres_ratio is not None else None)
        o = self.out
        self.B = B
        self.args = _lib.pack(
            'mr_noc_decode_batched', **_decode_args(ap, ap_dt, i['labels'], i['flip'], i['dim'], i['dim_var'], r, num_classes, class_agnostic, self._keep, ref_length,
                                                    ref_focal_y, target_std, epistemic_std_gain, std_scale, epnp_ransac_thres_ratio),
            coords_2d=o['coords_2d'].data_ptr(), coords_2d_istd=o['coords_2d_istd'].data_ptr(), coords_3d=o['coords_3d'].data_ptr(), dims=o['dims'].data_ptr(),
            dims_var=_lib.ptr(o['dims_var']), ransac_thr=_lib.ptr(o['ransac_thr']), **_coord_map_args(cmap))

    def run(self, stream=None):
        if self.B:
            with torch.cuda.device(self.dev):
                st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
                code = self.lib.mr_noc_decode_batched(*self.args, st)
                if code:
                    _lib.check(code)
        return self.out


def pnp_from_head(all_pred, labels, flip, dim, dim_var, rois, cam_intrinsic, img_shapes, num_classes=3, class_agnostic=False,
                  dim_means=DIM_MEANS, dim_stds=DIM_STDS, noc_means=NOC_MEANS, noc_stds=NOC_STDS,
                  ref_length=1.6, ref_focal_y=722, target_std=0.15, epistemic_std_gain=1.0, std_scale=10,
                  epnp_ransac_thres_ratio=0.2, allowed_border=200, z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True,
                  flags=0, with_diag=False, coord_2d=None, cov_calib_logscale=None, cov_correction_sd=0.0):
    """Raw NOC-head output -> (ret_val, yaw, t_vec, pose_cov, inlier_mask, dims, dims_var[, diag][, pose_cov_calib]) in ONE
    launch (``mr_pnp_from_head_batched``): the decoded 2D/3D/istd maps only ever exist in the kernel's LDS tile.
    cov_calib_logscale (4,): also return the calibrated covariance (s s^T) * cov (uncert_prop_pnp_optimizer.py:96-97),
    multiplied by (cov_correction_sd / ||t||)^2 when cov_correction_sd > 0 (monorun_roi_head.py:530-534)."""
    lib = _lib.load()
    dev = all_pred.device
    if dev.type != 'cuda':
        raise RuntimeError('monorun_amd.pnp_from_head runs on an MI355X only (no CPU fallback)')
    B, ch, h, w = all_pred.shape
    Cn = 1 if class_agnostic else num_classes
    assert ch == 2 * Cn * 5, f'all_pred has {ch} channels, expected {2 * Cn * 5}'
    f32t = torch.float32

    def prep(x, dt=f32t):                            # no-op for the tensors the pipeline already holds
        x = x.detach()
        if x.dtype != dt or x.device != dev:
            x = x.to(device=dev, dtype=dt)
        return x if x.is_contiguous() else x.contiguous()
    (ap, ap_dt), lab, dm = _head_output(all_pred, dev), prep(labels, torch.int64), prep(dim)
    fl = _flip_flags(flip, B, dev)
    dv = prep(dim_var) if dim_var is not None else None
    r = prep(rois)
    if r.shape[1] == 5:
        r = r[:, 1:5].contiguous()
    mu, sd, nm, ns = _const(dim_means, dev), _const(dim_stds, dev), _const(noc_means, dev), _const(noc_stds, dev)
    cam = prep(cam_intrinsic).reshape(-1, 3, 3)
    ur, vr = _clip_ranges(img_shapes, allowed_border, dev)
    P = h * w
    calib = cov_calib_logscale is not None
    # one float buffer and one byte buffer hold every output (two allocations per call)
    nf = 4 + 16 + 1 + 3 + (3 if dv is not None else 0) + (4 if with_diag else 0) + (16 if calib else 0)
    fbuf = torch.empty(max(B, 1) * nf, device=dev, dtype=f32t)
    bbuf = torch.empty(max(B, 1) * (1 + P), device=dev, dtype=torch.uint8)
    off = [0]

    def take(n):
        v = fbuf[off[0]:off[0] + B * n]
        off[0] += B * n
        return v
    pose, cov, tr, dims = take(4).view(B, 4), take(16).view(B, 4, 4), take(1), take(3).view(B, 3)
    dims_var = take(3).view(B, 3) if dv is not None else None
    diag = take(4).view(B, 4) if with_diag else None
    cov_calib = take(16).view(B, 4, 4) if calib else None
    valid, mask = bbuf[:B], bbuf[B:B + B * P].view(B, P)
    ls = prep(cov_calib_logscale) if calib else None
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_pnp_from_head_batched', **_decode_args(ap, ap_dt, lab, fl, dm, dv, r, num_classes, class_agnostic, (mu, sd, nm, ns),
                      ref_length, ref_focal_y, target_std, epistemic_std_gain, std_scale, epnp_ransac_thres_ratio), cam_mats=cam.data_ptr(),
                      cam_batch=cam.shape[0], u_range=ur.data_ptr(), v_range=vr.data_ptr(), range_batch=ur.shape[0], z_min=float(z_min),
                      istd_thres=float(epnp_istd_thres), inlier_opt_only=int(bool(inlier_opt_only)), flags=int(flags), valid=valid.data_ptr(),
                      pose=pose.data_ptr(), cov=cov.data_ptr(), tr_radius=tr.data_ptr(), inlier_mask=mask.data_ptr(), diag=_lib.ptr(diag),
                      dims=dims.data_ptr(), dims_var=_lib.ptr(dims_var), **_coord_map_args(_coord_map(coord_2d, dev)),
                      cov_calib_logscale=_lib.ptr(ls), cov_corr_sd=float(cov_correction_sd), cov_calib=_lib.ptr(cov_calib),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
    out = (valid.view(torch.bool), pose[:, :1], pose[:, 1:], cov, mask.view(torch.bool), dims, dims_var)
    if with_diag:
        out = out + (diag,)
    if calib:
        out = out + (cov_calib,)
    return out


_FLIP_CACHE = {}


def _flip_flags(flip, B, dev):
    """(B,) uint8 flip flags; the usual per-image bool (Python / numpy bool or a 0-dim / 1-element tensor or array, as
    img_meta['flip'] arrives) becomes a cached constant tensor; anything else must hold exactly B flags."""
    if torch.is_tensor(flip) and flip.numel() == 1 and B != 1:
        flip = bool(flip.item())
    elif isinstance(flip, np.ndarray) and flip.size == 1 and B != 1:
        flip = bool(flip.reshape(()))
    if isinstance(flip, (bool, np.bool_)):
        key = (str(dev), bool(flip), B)
        t = _FLIP_CACHE.get(key)
        if t is None:
            if len(_FLIP_CACHE) > 64:
                _FLIP_CACHE.clear()
            t = torch.full((max(B, 1),), int(flip), device=dev, dtype=torch.uint8)
            _FLIP_CACHE[key] = t
        return t
    fl = torch.as_tensor(flip, device=dev).to(torch.uint8).reshape(-1).contiguous()
    assert fl.numel() == B, f'flip must be a bool or hold one flag per object ({B}), got {fl.numel()}'
    return fl


def _planar_view(x):
    """(B,C,h,w) -> (B, h*w, C) strided view; point index p = y*w + x (uncert_prop_pnp_optimizer.py:82-84)."""
    b, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).view(b, h * w, c)


def cov_correction(cov, t_vec, ref_length=1.6, ref_focal_y=722, target_std=0.15):
    sd = ref_length * ref_focal_y * target_std
    return cov * (sd / torch.norm(t_vec, p=2, dim=1)).square().view(-1, 1, 1)


class Vec2DRotationCoder:
    """yaw (n, 1) -> (cos, sin) (n, 2) (the reference's core/bbox_3d/rotation_coder/vec2d_rotation_coder.py)."""

    @staticmethod
    def encode(angles):
        if angles.dim() == 1:
            angles = angles.unsqueeze(-1)
        return torch.cat((torch.cos(angles), torch.sin(angles)), dim=-1)


class UncertPropPnPOptimizer(nn.Module):
    """Pose head.  Constructor keywords follow the reference so that the ``pose_head`` dict of the shipped configs builds unchanged.
    Loss dicts are built as the reference builds them (``losses.build_loss``: mmdet's registry when it imports, else this package's)
    and stay plain assignable attributes, as ``LossUpdaterHook`` expects; a type no registry knows raises only when ``loss()``
    calls it.  The losses add no parameters or buffers: ``state_dict()`` is that of the inference head."""

    def __init__(self, loss_rot=None, loss_trans=None, loss_calib=None,
                 rotation_coder=dict(type='Vec2DRotationCoder'),
                 pnp=dict(type='PnPUncert', z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True,
                          forward_exact_hessian=False),
                 allowed_border=200, epnp_ransac_thres_ratio=0.2, std_scale=10):
        super().__init__()
        self.pnp = build_pnp(pnp)
        self.rotation_coder = Vec2DRotationCoder() if (rotation_coder or {}).get('type') == 'Vec2DRotationCoder' else None
        self.rotation_coder_cfg = rotation_coder
        self.loss_rot = build_loss(loss_rot)
        self.loss_trans = build_loss(loss_trans)
        self.loss_calib = build_loss(loss_calib)
        if getattr(self.pnp, 'use_6dof', False):
            # the reference never reads this flag (pnp_uncert.py:11): inside the head the pose stays [yaw, t] with a 4x4 covariance
            # (calibration and score head are 4-DoF); the real 6-DoF refinement is ops.pnp_uncert(..., use_6dof=True)
            warnings.warn('UncertPropPnPOptimizer: use_6dof is ignored inside the pose head (as in the reference)')
            self.pnp.use_6dof = False
        self.epnp_ransac_thres_ratio = epnp_ransac_thres_ratio
        self.allowed_border = allowed_border
        self.std_scale = std_scale
        self.cov_calib_logscale = nn.Parameter(torch.full((4, ), 0, dtype=torch.float))

    def init_weights(self):
        pass

    def _ranges(self, ref, img_shapes):
        n = img_shapes.size(0)
        u_range = ref.new_full((n, 2), -self.allowed_border)
        v_range = ref.new_full((n, 2), -self.allowed_border)
        u_range[:, 1] = img_shapes[:, 1] + self.allowed_border
        v_range[:, 1] = img_shapes[:, 0] + self.allowed_border
        return u_range, v_range

    def _calibrate(self, pose_cov):
        s = torch.exp(self.cov_calib_logscale)
        return (s * s[:, None]) * pose_cov

    def forward(self, coords_2d, coords_2d_logstd, coords_3d, cam_intrinsic, img_shapes):
        """
        Args:
            coords_2d (Tensor): shape (Nbatch, 2, h, w)
            coords_2d_logstd (Tensor): shape (Nbatch, 2, h, w)
            coords_3d (Tensor): shape (Nbatch, 3, h, w)
            cam_intrinsic (Tensor): shape (Nbatch, 3, 3) or (1, 3, 3)
            img_shapes (torch.Tensor): Shape (Nbatch, 2) or (1, 2), [H, W]

        Returns:
            ret_val (Nbatch,) bool, yaw_pred (Nbatch,1), t_vec_pred (Nbatch,3),
            pose_cov_pred (Nbatch,4,4), pose_cov_calib (Nbatch,4,4)
        """
        istd = torch.exp(-coords_2d_logstd) / self.std_scale
        u_range, v_range = self._ranges(coords_2d, img_shapes)
        thr = None
        if self.epnp_ransac_thres_ratio is not None:
            thr = self.epnp_ransac_thres_ratio * (coords_2d[:, 1, -1, 0] - coords_2d[:, 1, 0, 0])
        ret_val, yaw, t_vec, pose_cov, _ = self.pnp(_planar_view(coords_2d), _planar_view(istd), _planar_view(coords_3d),
                                                    cam_intrinsic, u_range, v_range, thr)
        return ret_val, yaw, t_vec, pose_cov, self._calibrate(pose_cov)

    def forward_decoded(self, dec, cam_intrinsic, img_shapes, with_mask=False):
        """Same as ``forward`` but fed by ``noc_decode`` (istd and RANSAC threshold already on the device)."""
        u_range, v_range = self._ranges(dec['coords_2d'], img_shapes)
        ret_val, yaw, t_vec, pose_cov, mask = self.pnp(_planar_view(dec['coords_2d']), _planar_view(dec['coords_2d_istd']),
                                                    _planar_view(dec['coords_3d']), cam_intrinsic, u_range, v_range,
                                                    dec['ransac_thr'])
        out = (ret_val, yaw, t_vec, pose_cov, self._calibrate(pose_cov))
        return out + (mask,) if with_mask else out

    def get_targets(self, pos_bboxes_3d):
        """pos_bboxes_3d (n, 7) [l, h, w, x, y, z, ry] -> yaw_targets (n, 1), trans_targets (n, 3)."""
        return pos_bboxes_3d[:, 6:7], pos_bboxes_3d[:, 3:6]

    def loss(self, ret_val, yaw_pred, t_vec_pred, pose_cov, dimensions_pred, yaw_targets, trans_targets, pos_bboxes_3d, eps=1e-6):
        """The reference's pose loss (uncert_prop_pnp_optimizer.py:106-159).

        Args:
            ret_val (n,) bool, yaw_pred (n, 1), t_vec_pred (n, 3), pose_cov (n, 4, 4) (the calibrated covariance, as the RoI head
            passes it), dimensions_pred (n, 3), yaw_targets (n, 1), trans_targets (n, 3), pos_bboxes_3d (n, 7) [l, h, w, x, y, z, ry]

        Returns:
            (dict with 'mean_iou' and, for each loss module the head has, 'loss_rot' / 'loss_trans' / 'loss_calib';
             ious (n, 1): the 3-D IoU of predicted and target box, no grad, 0 for invalid objects — the score head's target)
        """
        half = (torch.float16, torch.bfloat16)
        yaw_pred, t_vec_pred, pose_cov, dimensions_pred = (t.float() if t.dtype in half else t for t in (yaw_pred, t_vec_pred, pose_cov, dimensions_pred))
        ret_val = ret_val.reshape(-1).bool()
        loss_pose = dict()
        with torch.no_grad():
            ious = bbox3d_overlaps_aligned(pos_bboxes_3d[:, [3, 4, 5, 0, 1, 2, 6]], torch.cat((t_vec_pred, dimensions_pred, yaw_pred), dim=1))
            ious[~ret_val] = 0
        loss_pose['mean_iou'] = ious.sum() if ious.size(0) == 0 else ious.mean()

        yaw_pred, yaw_targets = yaw_pred[ret_val], yaw_targets[ret_val]
        t_vec_pred, trans_targets = t_vec_pred[ret_val], trans_targets[ret_val]
        pose_cov = pose_cov[ret_val]
        if self.loss_rot is not None:
            if self.rotation_coder is None:
                raise RuntimeError(f'UncertPropPnPOptimizer.loss: loss_rot needs a Vec2DRotationCoder, got {self.rotation_coder_cfg!r}')
            rot_pred = self.rotation_coder.encode(yaw_pred)
            rot_targets = self.rotation_coder.encode(yaw_targets)
            if rot_pred.size(0) == 0:
                loss_pose['loss_rot'] = rot_pred.sum()
            else:
                loss_pose['loss_rot'] = self.loss_rot(torch.norm(rot_pred - rot_targets, dim=1, p=2, keepdim=True), -1)
        if self.loss_trans is not None:
            loss_pose['loss_trans'] = t_vec_pred.sum() if t_vec_pred.size(0) == 0 else self.loss_trans(t_vec_pred, trans_targets)
        if self.loss_calib is not None:
            if pose_cov.size(0) == 0:
                loss_pose['loss_calib'] = pose_cov.sum()
            else:
                with torch.no_grad():
                    yaw_diff = ((yaw_pred - yaw_targets) + np.pi) % (2 * np.pi) - np.pi
                    diff = torch.cat([yaw_diff, t_vec_pred - trans_targets], dim=1)
                inv_cov = torch.inverse(pose_cov + torch.eye(pose_cov.size(-1), dtype=pose_cov.dtype, device=pose_cov.device))
                loss_pose['loss_calib'] = self.loss_calib(diff, 0, inv_cov=inv_cov)
        return loss_pose, ious


def pose_from_head(pose_head, all_pred, labels, flip, dim, dim_var, rois, cam_intrinsic, img_shape,
                   apply_cov_correction=True, fused=True, **decode_kw):
    """NOC-head output -> pose results dict (what monorun_roi_head.py:509-534 produces).
    A head built from the reference's config dict runs the REFERENCE's flow (uncert_prop_pnp_optimizer.py:86-95 ->
    pnp_uncert_cpu.py:33-68): K2, the EPnP / RANSAC initialiser's launches, the LM launch.  A head whose ``pnp`` says
    ``initialiser='k0'`` (the fast mode) runs, with fused=True, ONE launch (decode inside the PnP kernel, this repository's initialiser
    K0), with fused=False K2 then the PnP kernel (two launches, the decoded maps are materialised) — bit-identical results.
    ``initialiser='epnp'``, ``forward_exact_hessian``, ``coord_istd_normalize`` or ``cov_symeig_rule`` take the K2 + module path
    whatever ``fused`` says."""
    p = pose_head.pnp
    if fused and (getattr(p, 'forward_exact_hessian', False) or getattr(p, 'coord_istd_normalize', False) or getattr(p, 'cov_symeig_rule', False)
                  or getattr(p, 'initialiser', 'epnp') != 'k0'):
        # options the one-launch kernel does not implement — among them the reference's own initialiser (initialiser='epnp': its
        # launches read the decoded maps) — take the module path, which honours them: K2, then PnPUncert.forward
        fused = False
    if fused:
        sd = decode_kw.get('ref_length', 1.6) * decode_kw.get('ref_focal_y', 722) * decode_kw.get('target_std', 0.15)
        ret_val, yaw, t_vec, cov, inlier_mask, dims, dims_var, cov_calib = pnp_from_head(
            all_pred, labels, flip, dim, dim_var, rois, cam_intrinsic, img_shape, std_scale=pose_head.std_scale,
            epnp_ransac_thres_ratio=pose_head.epnp_ransac_thres_ratio, allowed_border=pose_head.allowed_border,
            z_min=p.z_min, epnp_istd_thres=p.epnp_istd_thres, inlier_opt_only=p.inlier_opt_only,
            cov_calib_logscale=pose_head.cov_calib_logscale, cov_correction_sd=sd if apply_cov_correction else 0.0, **decode_kw)
        return dict(ret_val=ret_val, yaw_pred=yaw, t_vec_pred=t_vec, pose_cov_pred=cov, pose_cov_calib=cov_calib,
                    dimensions_pred=dims, dimensions_var=dims_var, inlier_mask=inlier_mask)      # calibration + distance correction done by the kernel
    else:
        dec = noc_decode(all_pred, labels, flip, dim, dim_var, rois, std_scale=pose_head.std_scale,
                         epnp_ransac_thres_ratio=pose_head.epnp_ransac_thres_ratio, **decode_kw)
        img_shapes = torch.as_tensor(np.asarray(_hw_rows(img_shape.cpu() if torch.is_tensor(img_shape) else img_shape), np.float32), device=all_pred.device)
        ret_val, yaw, t_vec, cov, cov_calib, inlier_mask = pose_head.forward_decoded(dec, cam_intrinsic, img_shapes, with_mask=True)
        dims, dims_var = dec['dims'], dec['dims_var']
    if apply_cov_correction:
        kw = {k: decode_kw[k] for k in ('ref_length', 'ref_focal_y', 'target_std') if k in decode_kw}
        cov_calib = cov_correction(cov_calib, t_vec, **kw)
    return dict(ret_val=ret_val, yaw_pred=yaw, t_vec_pred=t_vec, pose_cov_pred=cov, pose_cov_calib=cov_calib,
                dimensions_pred=dims, dimensions_var=dims_var, inlier_mask=inlier_mask)


class PoseFromHeadLaunch:
    """The per-image regime (monorun_roi_head.py:452: one image per forward, <= ~100 proposals): a PREPARED fused launch — or, for
    a head built with ``pnp.initialiser='epnp'`` (the reference's flow), the prepared sequence K2 -> EPnP / RANSAC -> LM.

    ``pose_from_head`` marshals ~60 ctypes arguments and allocates its outputs on every call (~40 us of host time, more than
    the kernel itself takes at B = 100).  Here every argument is built once over static input / output tensors;
    ``run()`` only enqueues the kernel on the current stream (a few us), and ``capture()`` records that launch into a HIP
    graph (``torch.cuda.CUDAGraph``) whose ``replay()`` costs one graph launch.  Usage is the usual static-buffer pattern:
    copy the new image's head output / labels / dims / RoIs into ``inputs`` (device-to-device, same stream), then
    ``run()`` or ``replay()``; the results are the tensors in ``out`` (same keys as ``pose_from_head``).
    Shapes (B, classes, h, w), the flip flag and the camera are fixed at construction."""

    def __init__(self, pose_head, all_pred, labels, flip, dim, dim_var, rois, cam_intrinsic, img_shape,
                 apply_cov_correction=True, flags=0, num_classes=3, class_agnostic=False, dim_means=DIM_MEANS, dim_stds=DIM_STDS,
                 noc_means=NOC_MEANS, noc_stds=NOC_STDS, ref_length=1.6, ref_focal_y=722, target_std=0.15, epistemic_std_gain=1.0,
                 coord_2d=None):
        self.lib = _lib.load()
        dev = all_pred.device
        if dev.type != 'cuda':
            raise RuntimeError('PoseFromHeadLaunch runs on an MI355X only (no CPU fallback)')
        self.dev = dev
        B, ch, h, w = all_pred.shape
        Cn = 1 if class_agnostic else num_classes
        assert ch == 2 * Cn * 5
        f32 = dict(device=dev, dtype=torch.float32)
        ap, ap_dt = _head_output(all_pred, dev)
        r = rois.detach().to(**f32)
        r = (r[:, 1:5] if r.shape[1] == 5 else r).contiguous()
        self.inputs = dict(all_pred=ap, labels=labels.detach().to(device=dev, dtype=torch.int64).contiguous(), flip=_flip_flags(flip, B, dev).clone(),
                           dim=dim.detach().to(**f32).contiguous(), dim_var=dim_var.detach().to(**f32).contiguous() if dim_var is not None else None,
                           rois=r, cam_intrinsic=cam_intrinsic.detach().to(**f32).reshape(-1, 3, 3).contiguous())
        ur, vr = _clip_ranges(img_shape, pose_head.allowed_border, dev)
        mu, sd, nm, ns = _const(dim_means, dev), _const(dim_stds, dev), _const(noc_means, dev), _const(noc_stds, dev)
        P = h * w
        p = pose_head.pnp
        if getattr(p, 'forward_exact_hessian', False) or getattr(p, 'coord_istd_normalize', False) or getattr(p, 'cov_symeig_rule', False):
            raise ValueError('PoseFromHeadLaunch prepares fixed launches: forward_exact_hessian / coord_istd_normalize / cov_symeig_rule '
                             'need pose_from_head (module path)')
        self._epnp = None
        if getattr(p, 'initialiser', 'epnp') == 'epnp':
            # the reference's initialiser: its launches read the decoded maps, so the prepared form is K2 (prepared) -> the initialiser's
            # launches + the LM launch (PnPEpnpLaunch) -> calibration / distance correction as three in-place tensor operations
            from .ops.least_squares.pnp_uncert import PnPEpnpLaunch
            k2 = NocDecodeLaunch(self.inputs['all_pred'], self.inputs['labels'], self.inputs['flip'], self.inputs['dim'], self.inputs['dim_var'], self.inputs['rois'],
                                 num_classes=num_classes, class_agnostic=class_agnostic, dim_means=dim_means, dim_stds=dim_stds, noc_means=noc_means,
                                 noc_stds=noc_stds, ref_length=ref_length, ref_focal_y=ref_focal_y, target_std=target_std,
                                 epistemic_std_gain=epistemic_std_gain, std_scale=pose_head.std_scale,
                                 epnp_ransac_thres_ratio=pose_head.epnp_ransac_thres_ratio, coord_2d=coord_2d)
            self.inputs['flip'] = k2.inputs['flip']                     # the one input K2 holds a private copy of: refresh THIS tensor
            self.inputs['coord_2d'] = k2.inputs['coord_2d']
            d = k2.out
            # the calibration reads the LIVE parameter on every run / replay (an alias of it when the head lives on the launch device in
            # float32, like the fused launch's): weights loaded or updated in place after this object was built are honoured, also by a
            # captured graph.  It is the LM launch's epilogue (mr_pnp_uncert_from_epnp_grouped: cov_calib), like the one-launch kernel's.
            ls = pose_head.cov_calib_logscale.detach().to(**f32).contiguous()
            sdc = float(ref_length * ref_focal_y * target_std) if apply_cov_correction else 0.0
            cov_calib = torch.empty(B, 4, 4, **f32)
            ep = PnPEpnpLaunch(_planar_view(d['coords_2d']), _planar_view(d['coords_2d_istd']), _planar_view(d['coords_3d']), self.inputs['cam_intrinsic'],
                               ur, vr, z_min=p.z_min, epnp_istd_thres=p.epnp_istd_thres, epnp_ransac_thres=d['ransac_thr'],
                               inlier_opt_only=p.inlier_opt_only, flags=flags, first_round=getattr(p, 'epnp_first_round', None), calib=(ls, sdc, cov_calib))
            self._epnp = dict(k2=k2, ep=ep, logscale=ls, sd=sdc)
            self.out = dict(ret_val_u8=ep.valid, pose=ep.pose, pose_cov_pred=ep.cov, tr_radius=ep.tr, inlier_mask_u8=ep.mask,
                            dimensions_pred=d['dims'], dimensions_var=d['dims_var'], pose_cov_calib=cov_calib)
            o = self.out
            o['ret_val'], o['inlier_mask'] = o['ret_val_u8'].view(torch.bool), o['inlier_mask_u8'].view(torch.bool)
            o['yaw_pred'], o['t_vec_pred'] = o['pose'][:, :1], o['pose'][:, 1:]
            self._keep = (ur, vr)
            self.B = B
            self.graph = None
            return
        self.out = dict(ret_val_u8=torch.empty(B, device=dev, dtype=torch.uint8), pose=torch.empty(B, 4, **f32), pose_cov_pred=torch.empty(B, 4, 4, **f32),
                        tr_radius=torch.empty(B, **f32), inlier_mask_u8=torch.empty(B, P, device=dev, dtype=torch.uint8),
                        dimensions_pred=torch.empty(B, 3, **f32), dimensions_var=torch.empty(B, 3, **f32) if dim_var is not None else None,
                        pose_cov_calib=torch.empty(B, 4, 4, **f32))
        o, i = self.out, self.inputs
        o['ret_val'], o['inlier_mask'] = o['ret_val_u8'].view(torch.bool), o['inlier_mask_u8'].view(torch.bool)
        o['yaw_pred'], o['t_vec_pred'] = o['pose'][:, :1], o['pose'][:, 1:]
        self.logscale = pose_head.cov_calib_logscale.detach().to(**f32).contiguous()
        sdv = ref_length * ref_focal_y * target_std
        # the map as the kernel reads it (a converted copy when coord_2d is fp16 / fp64 / on the host / non-contiguous): the
        # prepared launch holds it for as long as it lives; `inputs['coord_2d']` may be refreshed in place like the other inputs
        cmap = _coord_map(coord_2d, dev)
        self.inputs['coord_2d'] = cmap
        self._keep = (ur, vr, mu, sd, nm, ns, cmap)
        self.B = B
        cam = i['cam_intrinsic']
        self.args = _lib.pack(
            'mr_pnp_from_head_batched', **_decode_args(i['all_pred'], ap_dt, i['labels'], i['flip'], i['dim'], i['dim_var'], i['rois'], num_classes, class_agnostic,
                                                       (mu, sd, nm, ns), ref_length, ref_focal_y, target_std, epistemic_std_gain, pose_head.std_scale,
                                                       pose_head.epnp_ransac_thres_ratio),
            cam_mats=cam.data_ptr(), cam_batch=cam.shape[0], u_range=ur.data_ptr(), v_range=vr.data_ptr(), range_batch=ur.shape[0],
            z_min=float(p.z_min), istd_thres=float(p.epnp_istd_thres), inlier_opt_only=int(bool(p.inlier_opt_only)), flags=int(flags),
            valid=o['ret_val_u8'].data_ptr(), pose=o['pose'].data_ptr(), cov=o['pose_cov_pred'].data_ptr(), tr_radius=o['tr_radius'].data_ptr(),
            inlier_mask=o['inlier_mask_u8'].data_ptr(), diag=None, dims=o['dimensions_pred'].data_ptr(), dims_var=_lib.ptr(o['dimensions_var']),
            **_coord_map_args(cmap), cov_calib_logscale=self.logscale.data_ptr(), cov_corr_sd=float(sdv) if apply_cov_correction else 0.0, cov_calib=o['pose_cov_calib'].data_ptr())
        self.graph = None

    def run(self, stream=None):
        """Enqueue the launch on `stream` (a raw hipStream_t of THIS launch's device) or on that device's current stream.  The
        library launches on the current HIP device, so the device is made current for the call."""
        if self.B and self._epnp is not None:
            e = self._epnp
            with torch.cuda.device(self.dev):
                ts = torch.cuda.ExternalStream(stream, device=self.dev) if stream is not None else torch.cuda.current_stream(self.dev)
                e['k2'].run(ts.cuda_stream)
                e['ep'].run(ts.cuda_stream)                # (calibration / distance correction: the LM launch's epilogue)
        elif self.B:
            with torch.cuda.device(self.dev):
                st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
                code = self.lib.mr_pnp_from_head_batched(*self.args, st)
                if code:
                    _lib.check(code)
        return self.out

    def capture(self):
        """Record the launch into a HIP graph (one warm-up launch first: the LDS opt-in of the kernel is set outside the capture)."""
        with torch.cuda.device(self.dev):
            self.run()
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.run()
        self.graph = g
        return self

    def replay(self):
        if self.graph is None:
            self.capture()
        with torch.cuda.device(self.dev):
            self.graph.replay()
        return self.out


class PoseFromHeadGroupLaunch:
    """Up to eight prepared ``PoseFromHeadLaunch`` objects of the REFERENCE flow (heads built with the default initialiser) and the same
    shape as ONE launch set: every member's K2 decode, then the initialiser's launches and the re-fit / LM launch over the objects of all
    members (``PnPEpnpGroupLaunch``; calibration in its epilogue) — all on the stream ``run`` is given.  Members keep their inputs
    and outputs; results are bit-identical to running them one by one.  The regime a serving loop with several images' proposals at
    hand wants (the stages are latency chains, HIP runs the launches of four streams side by side)."""

    def __init__(self, launches):
        from .ops.least_squares.pnp_uncert import PnPEpnpGroupLaunch
        self.members = list(launches)
        if not self.members or any(m._epnp is None for m in self.members):
            raise ValueError("PoseFromHeadGroupLaunch groups launches of the reference flow (pnp.initialiser='epnp', the default)")
        self.dev = self.members[0].dev
        self.set = PnPEpnpGroupLaunch([m._epnp['ep'] for m in self.members])

    def run(self, stream=None):
        with torch.cuda.device(self.dev):
            ts = torch.cuda.ExternalStream(stream, device=self.dev) if stream is not None else torch.cuda.current_stream(self.dev)
            for m in self.members:
                if m.B:
                    m._epnp['k2'].run(ts.cuda_stream)
            self.set.run(ts.cuda_stream)
        return [m.out for m in self.members]
