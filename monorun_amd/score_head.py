"""The score head (N7): ``MLPScoreHead`` with its ``BatchNormSmooth1D``, and ``IoU3DBalancedSampler``, of the reference
(monorun/models/roi_heads/bbox_3d_heads/score_heads/mlp_score_head.py, monorun/core/bbox_3d/samplers/iou3d_balanced_sampler.py),
without mmdet, and the scoring step of the RoI head's test path (monorun_roi_head.py:536-550) as ``score_poses``.

The module is torch on any device: training runs the torch ops (three small ``Linear`` layers; there is no HIP backward).  At
inference — the head in eval mode, on a HIP device, in the configuration every shipped config uses (``fused_ok()``) —
``score_poses`` makes ONE launch (``mr_score_head_forward``, include/monorun_heads.h): gather of the 17 inputs, the norm, both
hidden layers, the output layer, the sigmoid, the mask of failed solves and the 2-D score multiply.  The fused launch is forward
only: its result carries no graph.  ``ScoreHeadLaunch`` is its prepared, static-buffer form (``run`` / ``capture`` / ``replay``).
"""
import torch
import torch.nn as nn
from torch.nn.modules.batchnorm import _NormBase

from . import _lib
from .consumers import score_head_inputs
from .losses import build_loss

ROWS_PER_WORKGROUP = 4          # rows of one workgroup's tile (kScoreRows of csrc/score_head_kernel.inc)
MAX_C1, MAX_C2 = 2048, 1024     # MR_SCORE_MAX_C1 / MR_SCORE_MAX_C2 of include/monorun_heads.h
POSE_DIM = 1 + 3 + 10 + 3       # yaw, t_vec, lower triangle of the 4 x 4 covariance, dimensions


class BatchNormSmooth1D(_NormBase):
    """Batch norm that ALWAYS normalises with the running statistics: buffers and parameters have the names and shapes of
    ``torch.nn.BatchNorm1d``.  In training mode with more than one row it first folds ``var_mean(input, dim=0)`` (unbiased
    variance) into the running statistics; with one row, or in eval mode, it only normalises.  ``num_batches_tracked`` counts
    every training call.

    The statistic update runs under ``torch.no_grad()``: the buffers never join the graph, so no gradient reaches the input
    through them.  (The reference updates them in place outside ``no_grad``; its inputs are detached there, so nothing differs
    in the shipped configuration.)"""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        if not track_running_stats:
            raise ValueError('BatchNormSmooth1D normalises with the running statistics: track_running_stats must be True')
        super().__init__(num_features, eps, momentum, affine, track_running_stats)

    def forward(self, input):
        if input.dim() != 2:
            raise ValueError(f'expected 2D input (got {input.dim()}D input)')
        if self.training:
            with torch.no_grad():
                self.num_batches_tracked += 1
                factor = self.momentum if self.momentum is not None else 1.0 / float(self.num_batches_tracked)
                if input.size(0) > 1:
                    var, mean = torch.var_mean(input.detach(), dim=0)
                    self.running_mean *= 1 - factor
                    self.running_mean += factor * mean
                    self.running_var *= 1 - factor
                    self.running_var += factor * var
        out = input.sub(self.running_mean).div((self.running_var + self.eps).sqrt())
        if self.affine:
            out = out.mul(self.weight).add(self.bias)
        return out


class IoU3DBalancedSampler:
    """Keeps the share of positives (``ious >= pos_iou_thr``) among the sampled elements within
    [``pos_fraction_min``, ``pos_fraction_max``] by dropping elements of the class in excess at random.  With ``smooth_keeprate``
    the keep rate is a linear function of the IoU through the two classes' rates at the strong thresholds; it is NOT clamped to
    the two rates (the reference computes the clamp and discards its result), so it may leave [0, 1]."""

    def __init__(self, pos_iou_thr=0.5, pos_fraction_min=0.25, pos_fraction_max=0.75, smooth_keeprate=True, min_iou=-1):
        self.pos_iou_thr = pos_iou_thr
        self.pos_fraction_min = pos_fraction_min
        self.pos_fraction_max = pos_fraction_max
        self.smooth_keeprate = smooth_keeprate
        self.min_iou = min_iou

    def keeprate(self, ious):
        """None when every element is kept, else the per-element keep rate (the shape of ``ious``)."""
        pos_mask = ious >= self.pos_iou_thr
        num_pos = torch.sum(pos_mask)
        num_neg = ious.numel() - num_pos
        num_pos_max = self.pos_fraction_max / (1 - self.pos_fraction_max) * num_neg
        num_neg_max = (1 - self.pos_fraction_min) / self.pos_fraction_min * num_pos
        if num_pos <= num_pos_max and num_neg <= num_neg_max:
            return None
        if num_pos > num_pos_max:
            pos_rate, neg_rate = num_pos_max / num_pos, 1
        else:
            pos_rate, neg_rate = 1, num_neg_max / num_neg
        if not self.smooth_keeprate:
            rate = torch.full_like(ious, float(neg_rate))
            rate[pos_mask] = float(pos_rate)
            return rate
        strong_pos_thr = (self.pos_iou_thr + 1) / 2
        strong_neg_thr = self.pos_iou_thr / 2
        return (pos_rate - neg_rate) / (strong_pos_thr - strong_neg_thr) * (ious - strong_neg_thr) + neg_rate

    def sample(self, ious):
        rate = self.keeprate(ious)
        mask = torch.ones_like(ious, dtype=torch.bool) if rate is None else torch.rand_like(ious) < rate
        mask[ious < self.min_iou] = 0
        return mask


IOU3D_SAMPLERS = {'IoU3DBalancedSampler': IoU3DBalancedSampler}


def build_iou3d_sampler(cfg):
    cfg = dict(cfg)
    typ = cfg.pop('type')
    if typ not in IOU3D_SAMPLERS:
        raise ValueError(f'unknown IoU sampler {typ!r}')
    return IOU3D_SAMPLERS[typ](**cfg)


def _cfg_get(cfg, key):
    """``cfg[key]`` of a dict or ``cfg.key`` of an attribute object; None when absent."""
    if not cfg:
        return None
    if isinstance(cfg, dict):
        return cfg.get(key)
    return getattr(cfg, key, None)


class MLPScoreHead(nn.Module):
    """The reference's score head: same constructor arguments and defaults, same ``state_dict`` keys and shapes (``pose_norm.*``,
    ``pose_fcs.N.*``, ``fused_fcs.N.*``, ``fc_out.*``), so ``roi_head.score_head.*`` of a MonoRUn checkpoint loads with
    ``strict=True``.  ``forward`` returns logits (``pre_sigmoid``)."""

    def __init__(self,
                 reg_fc_out_channels=1024,
                 num_pose_fcs=1,
                 pose_fc_out_channels=1024,
                 fusion_type='add',
                 num_fused_fcs=1,
                 fc_out_channels=256,
                 loss_score=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 mode='linear_average',
                 iou_thres=0.7,
                 linear_coefs=(-0.5, 2),
                 detach_preds=True,
                 use_pose_norm=True,
                 train_cfg=None):
        super().__init__()
        if mode not in ('average', 'thres', 'linear_average'):
            raise ValueError(f'mode must be "average", "thres" or "linear_average", not {mode!r}')
        if fusion_type not in ('add', 'concat'):
            raise ValueError(f'fusion_type must be "add" or "concat", not {fusion_type!r}')
        if num_pose_fcs < 1 or num_fused_fcs < 1:
            raise ValueError('num_pose_fcs and num_fused_fcs must be at least 1')
        if fusion_type == 'add' and pose_fc_out_channels != reg_fc_out_channels:
            raise ValueError("fusion_type='add' needs pose_fc_out_channels == reg_fc_out_channels")
        self.num_pose_fcs = num_pose_fcs
        self.num_fused_fcs = num_fused_fcs
        self.fc_out_channels = fc_out_channels
        self.pose_fc_out_channels = pose_fc_out_channels
        self.mode = mode
        self.iou_thres = iou_thres
        self.linear_coefs = linear_coefs
        self.fp16_enabled = False
        self.loss_score = build_loss(loss_score) if loss_score is not None else None
        self.relu = nn.ReLU(inplace=True)
        self.pre_sigmoid = True
        self.detach_preds = detach_preds
        self.reg_fc_out_channels = reg_fc_out_channels
        self.fusion_type = fusion_type
        self.use_pose_norm = use_pose_norm
        self.train_cfg = train_cfg
        sampler = _cfg_get(train_cfg, 'iou3d_sampler')
        self.iou3d_sampler = build_iou3d_sampler(sampler) if sampler is not None else None

        self.pose_fcs = nn.ModuleList()                 # registered before pose_norm: the reference's state_dict order
        if use_pose_norm:
            self.pose_norm = BatchNormSmooth1D(POSE_DIM, momentum=0.01)
        self.pose_fcs.extend(nn.Linear(POSE_DIM if i == 0 else pose_fc_out_channels, pose_fc_out_channels) for i in range(num_pose_fcs))
        fused_in = reg_fc_out_channels + (pose_fc_out_channels if fusion_type == 'concat' else 0)
        self.fused_fcs = nn.ModuleList(nn.Linear(fused_in if i == 0 else fc_out_channels, fc_out_channels) for i in range(num_fused_fcs))
        self.fc_out = nn.Linear(fc_out_channels, 1)
        self._packed = {}

    def init_weights(self):
        for fc in list(self.pose_fcs) + list(self.fused_fcs):
            nn.init.xavier_uniform_(fc.weight)
            nn.init.constant_(fc.bias, 0)
        nn.init.normal_(self.fc_out.weight, 0, 0.01)
        nn.init.constant_(self.fc_out.bias, 0)

    def forward(self, reg_fc_out, yaw, t_vec, pose_cov, dimensions):
        """reg_fc_out (n, reg_fc_out_channels), yaw (n, 1), t_vec (n, 3), pose_cov (n, 4, 4), dimensions (n, 3) -> (n,) logits."""
        if self.detach_preds:
            yaw, t_vec, pose_cov, dimensions = yaw.detach(), t_vec.detach(), pose_cov.detach(), dimensions.detach()
        x = score_head_inputs(yaw, t_vec, pose_cov, dimensions)
        if self.use_pose_norm:
            x = self.pose_norm(x)
        for fc in self.pose_fcs:
            x = self.relu(fc(x))
        x = x + reg_fc_out if self.fusion_type == 'add' else torch.cat([x, reg_fc_out], dim=1)
        for fc in self.fused_fcs:
            x = self.relu(fc(x))
        return self.fc_out(x).squeeze(1)

    def get_targets(self, ious):
        """The score target of an IoU: the IoU itself ('average'), its threshold indicator ('thres') or a clamped linear map."""
        if self.mode == 'thres':
            return (ious >= self.iou_thres).to(ious.dtype)
        if self.mode == 'linear_average':
            return (self.linear_coefs[0] + ious * self.linear_coefs[1]).clamp_(min=0, max=1)
        return ious

    def loss(self, scores, ious):
        """scores (n,) logits, ious (n, 1) -> dict(loss_score=...).  With a sampler the loss is weighted per sample by the sampling
        mask over its mean (clamped at 1e-2).  n = 0: a zero that keeps the graph."""
        if self.loss_score is None:
            return dict()
        if scores.size(0) == 0:
            return dict(loss_score=scores.sum())
        scores = scores.unsqueeze(1)
        targets = self.get_targets(ious).to(scores.dtype)
        if self.iou3d_sampler is None:
            return dict(loss_score=self.loss_score(scores, targets))
        weight = self.iou3d_sampler.sample(ious).to(ious.dtype)
        weight /= weight.mean().clamp(min=1e-2)
        return dict(loss_score=self.loss_score(scores, targets, weight=weight))

    # ------------------------------------------------------------------------------------------------- the fused launch
    def fused_ok(self):
        """Whether the one-launch kernel covers this configuration: one pose layer, one fused layer, fusion by addition, channel
        counts within the kernel's limits (every config file of the reference)."""
        return (self.num_pose_fcs == 1 and self.num_fused_fcs == 1 and self.fusion_type == 'add'
                and 1 <= self.pose_fc_out_channels <= MAX_C1 and 1 <= self.fc_out_channels <= MAX_C2)

    def _tensors(self):
        return list(self.parameters()) + list(self.buffers())

    def packed_params(self, device):
        """The kernel's parameter buffer on ``device`` (layout: include/monorun_heads.h), fp32.  Cached; the key is the device and
        every parameter's and buffer's storage and ``_version`` counter, so an in-place change (an optimizer step, a loaded
        state_dict) or a moved module rebuilds it on the next call."""
        device = torch.device(device)
        key = tuple((t.data_ptr(), t._version) for t in self._tensors())
        hit = self._packed.get(device)
        if hit is None or hit[0] != key:
            hit = (key, pack_params(self, device))
            self._packed[device] = hit
        return hit[1]


def packed_numel(c1, c2):
    r4 = lambda v: (v + 3) // 4 * 4
    return 64 + r4(POSE_DIM * c1) + r4(c1) + c1 * r4(c2) + 2 * r4(c2) + 4


@torch.no_grad()
def pack_params(head, device):
    """One fp32 buffer with the norm folded to (mean, scale, shift) and W1, W2 transposed, as mr_score_head_forward reads it."""
    if not head.fused_ok():
        raise ValueError('pack_params: the fused kernel does not cover this MLPScoreHead configuration (fused_ok() is False)')
    f32 = dict(device=device, dtype=torch.float32)
    c1, c2 = head.pose_fc_out_channels, head.fc_out_channels
    c2p = (c2 + 3) // 4 * 4
    r4 = lambda v: (v + 3) // 4 * 4
    buf = torch.zeros(packed_numel(c1, c2), **f32)
    if head.use_pose_norm:
        norm = head.pose_norm
        scale = (norm.running_var.to(**f32) + norm.eps).sqrt().reciprocal()
        if norm.affine:
            scale = norm.weight.to(**f32) / (norm.running_var.to(**f32) + norm.eps).sqrt()
            buf[2 * POSE_DIM:3 * POSE_DIM] = norm.bias.to(**f32)
        buf[0:POSE_DIM] = norm.running_mean.to(**f32)
        buf[POSE_DIM:2 * POSE_DIM] = scale
    else:
        buf[POSE_DIM:2 * POSE_DIM] = 1
    o = 64
    fc1, fc2 = head.pose_fcs[0], head.fused_fcs[0]
    buf[o:o + POSE_DIM * c1] = fc1.weight.to(**f32).t().reshape(-1)
    o += r4(POSE_DIM * c1)
    buf[o:o + c1] = fc1.bias.to(**f32)
    o += r4(c1)
    buf[o:o + c1 * c2p].view(c1, c2p)[:, :c2] = fc2.weight.to(**f32).t()
    o += c1 * c2p
    buf[o:o + c2] = fc2.bias.to(**f32)
    o += c2p
    buf[o:o + c2] = head.fc_out.weight.to(**f32).reshape(-1)
    o += c2p
    buf[o] = head.fc_out.bias.to(**f32)[0]
    return buf


def _rows(t, width):
    """fp32 (n, width) rows the kernel reads in place: unit column stride, any row stride >= width (views of wider tensors)."""
    t = t.detach().to(torch.float32)
    if t.dim() != 2 or t.size(1) != width:
        raise ValueError(f'expected (n, {width}), got {tuple(t.shape)}')
    return t if t.size(0) == 0 or (t.stride(1) == 1 and t.stride(0) >= width) or (width == 1 and t.stride(0) >= 1) else t.contiguous()


def _score_args(head, reg, yaw, t_vec, cov, dims, ret_val_u8, scores_2d, params, out, flags):
    """The arguments of ``mr_score_head_forward`` by name."""
    n = reg.size(0)
    return dict(reg_fc_out=reg.data_ptr(), reg_fc_out_row_stride=max(reg.stride(0), reg.size(1)),
                yaw=yaw.data_ptr(), yaw_row_stride=max(yaw.stride(0), 1), t_vec=t_vec.data_ptr(), t_vec_row_stride=max(t_vec.stride(0), 3),
                pose_cov=cov.data_ptr(), dimensions=dims.data_ptr(), dimensions_row_stride=max(dims.stride(0), 3),
                ret_val=_lib.ptr(ret_val_u8), scores_2d=_lib.ptr(scores_2d), params=params.data_ptr(), params_numel=params.numel(),
                n=n, c1=head.pose_fc_out_channels, c2=head.fc_out_channels, flags=flags, scores=out.data_ptr())


def score_head_forward_fused(head, reg_fc_out, yaw, t_vec, pose_cov, dimensions, ret_val=None, scores_2d=None, sigmoid=True):
    """ONE launch of ``mr_score_head_forward`` on the inputs' device: (n,) fp32 scores (logits with ``sigmoid=False``), 0 where
    ``ret_val`` is False, times ``scores_2d`` where given.  Forward only.  A configuration the kernel does not cover or a
    device that is not a HIP device is an error, never a fall-back."""
    dev = reg_fc_out.device
    if dev.type != 'cuda':
        raise RuntimeError('score_head_forward_fused runs on an MI355X only (no CPU fallback)')
    _lib.load()
    f32 = dict(device=dev, dtype=torch.float32)
    n = reg_fc_out.size(0)
    reg = _rows(reg_fc_out, head.reg_fc_out_channels)
    yaw, t_vec, dims = _rows(yaw, 1), _rows(t_vec, 3), _rows(dimensions, 3)
    cov = pose_cov.detach().to(**f32).reshape(n, 4, 4).contiguous()
    rv = ret_val.detach().reshape(n).to(torch.bool).contiguous().view(torch.uint8) if ret_val is not None else None
    s2d = scores_2d.detach().to(**f32).reshape(n).contiguous() if scores_2d is not None else None
    out = torch.empty(n, **f32)
    params = head.packed_params(dev)
    with torch.cuda.device(dev):
        _lib.call('mr_score_head_forward', _score_args(head, reg, yaw, t_vec, cov, dims, rv, s2d, params, out, _lib.MR_SCORE_SIGMOID if sigmoid else 0),
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    return out


def score_poses_torch(score_head, reg_fc_out, pose_results, dimensions=None, det_scores=None, calib_scoring=True, mult_2d_score=True):
    """The scoring step of the RoI head's test path in torch ops (monorun_roi_head.py:536-550), on any device."""
    cov = pose_results['pose_cov_calib'] if calib_scoring else pose_results['pose_cov_pred']
    dims = pose_results['dimensions_pred'] if dimensions is None else dimensions
    scores = score_head(reg_fc_out, pose_results['yaw_pred'], pose_results['t_vec_pred'], cov, dims)
    if score_head.pre_sigmoid:
        scores = scores.sigmoid()
    scores = scores.masked_fill(~pose_results['ret_val'].reshape(-1).bool(), 0)
    return det_scores * scores if mult_2d_score else scores


def score_poses(score_head, reg_fc_out, pose_results, dimensions=None, det_scores=None, calib_scoring=True, mult_2d_score=True):
    """Pose results dict of ``pose_from_head`` -> (n,) 3-D scores: the score head on ``pose_cov_calib`` (``calib_scoring``) or
    ``pose_cov_pred``, the sigmoid, 0 where the solve failed (``~ret_val``), times the 2-D detection score ``det_scores`` (n,)
    with ``mult_2d_score`` (monorun_roi_head.py:536-550; ``dimensions`` defaults to ``pose_results['dimensions_pred']``).

    On a HIP device, with the head in eval mode and ``score_head.fused_ok()``, this is one launch (no graph is kept); otherwise
    the torch ops of :func:`score_poses_torch`."""
    if mult_2d_score and det_scores is None:
        raise ValueError('score_poses: mult_2d_score needs det_scores')
    if reg_fc_out.device.type == 'cuda' and not score_head.training and score_head.fused_ok() and score_head.pre_sigmoid:
        cov = pose_results['pose_cov_calib'] if calib_scoring else pose_results['pose_cov_pred']
        dims = pose_results['dimensions_pred'] if dimensions is None else dimensions
        out = score_head_forward_fused(score_head, reg_fc_out, pose_results['yaw_pred'], pose_results['t_vec_pred'], cov, dims,
                                       ret_val=pose_results['ret_val'], scores_2d=det_scores if mult_2d_score else None)
        return out.to(reg_fc_out.dtype)
    return score_poses_torch(score_head, reg_fc_out, pose_results, dimensions, det_scores, calib_scoring, mult_2d_score)


class ScoreHeadLaunch:
    """The prepared, static-buffer form of the fused launch (the pattern of ``PoseFromHeadLaunch``): every argument is built once
    over the tensors in ``inputs`` (reg_fc_out, yaw, t_vec, pose_cov, dimensions, ret_val_u8, and det_scores with
    ``mult_2d_score``) and ``out`` (scores).  Copy a new image's values into ``inputs`` on the same stream, then ``run()`` —
    exactly one launch enqueued on the current stream, nothing on the host that synchronises — or ``replay()`` of the graph
    ``capture()`` recorded.  ``n`` and the head's parameters are fixed at construction: the launch holds the parameter buffer
    packed then (``refresh_params()`` re-packs into the same memory after the weights changed)."""

    def __init__(self, score_head, n, device, mult_2d_score=True, sigmoid=True):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('ScoreHeadLaunch runs on an MI355X only (no CPU fallback)')
        if score_head.training or not score_head.fused_ok():
            raise ValueError('ScoreHeadLaunch prepares the fused launch: the head must be in eval mode and fused_ok()')
        self.lib = _lib.load()
        self.head, self.dev, self.n = score_head, device, int(n)
        f32 = dict(device=device, dtype=torch.float32)
        self.inputs = dict(reg_fc_out=torch.zeros(n, score_head.reg_fc_out_channels, **f32), yaw=torch.zeros(n, 1, **f32),
                           t_vec=torch.zeros(n, 3, **f32), pose_cov=torch.zeros(n, 4, 4, **f32), dimensions=torch.zeros(n, 3, **f32),
                           ret_val_u8=torch.ones(n, device=device, dtype=torch.uint8),
                           det_scores=torch.ones(n, **f32) if mult_2d_score else None)
        self.inputs['ret_val'] = self.inputs['ret_val_u8'].view(torch.bool)
        self.out = dict(scores=torch.zeros(n, **f32))
        self.params = score_head.packed_params(device).clone()
        i = self.inputs
        self.args = _lib.pack('mr_score_head_forward', _score_args(
            score_head, i['reg_fc_out'], i['yaw'], i['t_vec'], i['pose_cov'], i['dimensions'], i['ret_val_u8'], i['det_scores'], self.params,
            self.out['scores'], _lib.MR_SCORE_SIGMOID if sigmoid else 0))
        self.graph = None

    def refresh_params(self):
        self.params.copy_(self.head.packed_params(self.dev))
        return self

    def run(self, stream=None):
        """Enqueue the launch on `stream` (a raw hipStream_t of this launch's device) or on that device's current stream."""
        if self.n:
            with torch.cuda.device(self.dev):
                st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
                code = self.lib.mr_score_head_forward(*self.args, st)
                if code:
                    _lib.check(code)
        return self.out

    def capture(self):
        """Record the launch into a HIP graph (one warm-up launch first, outside the capture)."""
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
