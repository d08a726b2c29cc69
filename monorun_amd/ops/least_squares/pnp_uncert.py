"""Torch-facing uncertainty-aware PnP op — drop-in for
/root/reference/monorun/ops/least_squares/pnp_uncert.py (``pnp_uncert`` :7-87, ``PnPUncert`` :90-142).

Same names, argument meaning, return tuple, dtypes and devices.  What differs is the execution:
the reference copies six tensors to the host, loops over objects in Python (cv2 EPnP/RANSAC + cffi
Ceres LM), copies back and builds J^T J with ~40 small torch kernels; here ONE fused HIP kernel
(``mr_pnp_uncert_batched`` in include/monorun_pnp.h) does mask -> initialiser -> LM -> covariance on the
device, on the caller's stream, with no host synchronisation.
"""
import ctypes

import torch

from ... import _lib
from .builder import PNP

_DTYPES = {torch.float32: _lib.MR_F32, torch.float16: _lib.MR_F16, torch.float64: _lib.MR_F64}

# What `build_pnp(dict(type='PnPUncert', ...))` from the reference's own config dict, `pnp_uncert`, `u2d_pnp_cpu` and the pose head run when
# nobody says otherwise: the REFERENCE's flow — cv2.solvePnPRansac(EPNP, 30 iterations) restated on the GPU, then the LM + covariance
# (pnp_uncert_cpu.py:33-68).  'k0' (this repository's one-launch consensus initialiser: ~5 x the throughput, the same LM, inlier sets that
# differ from the reference flow's on ~13 % of the objects) is an explicit fast mode since round 5.
DEFAULT_INITIALISER = 'epnp'

# the bits of a call's flags that the initialiser reads
_INIT_FLAGS = _lib.MR_MEAN_MASK | _lib.MR_NO_ISTD_MASK | _lib.MR_EPNP_REFIT_F32 | _lib.MR_EPNP_CV_EARLY_RETURN


def _strides(t):
    return (ctypes.c_int64 * 3)(*t.stride())


def _first_round_flags(flags, first_round):
    """`flags` with first_round (None: as it is) in its first-round field: the hypotheses solved for every object before the replayed loop
    is consulted (1..30; result-neutral)."""
    if first_round is None:
        return int(flags)
    return (int(flags) & ~(0x1F << _lib.MR_EPNP_FIRST_ROUND_SHIFT)) | (max(1, min(30, int(first_round))) << _lib.MR_EPNP_FIRST_ROUND_SHIFT)


def _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range=None, v_range=None, ransac_thr=None, init_pose=None, no_gpu=None,
            prepared=False):
    """The inputs every entry point shares.  Returns (dev, B, P, common, keep): `common` = the arguments the prototypes share, under the
    header's names (x2d ... in_dtype, cam_mats, cam_batch and, with u_range / v_range, those and range_batch), for ``_lib.pack``; `keep` = the
    tensors they point into plus ransac_thr f32 (n,) | None and init_pose f64 (n,4) | None, which whoever launches must keep alive.
    The coordinate tensors are detached and converted to the storage dtype (their own where the kernels read it, else float32) on the
    device of coords_2d; prepared=True (the launch classes) asserts their dtypes instead and aliases the caller's buffers.
    no_gpu: the RuntimeError message when coords_2d is not on a HIP device (None: not checked here)."""
    dev = coords_2d.device
    if no_gpu is not None and dev.type != 'cuda':
        raise RuntimeError(no_gpu)
    B, P = int(coords_2d.shape[0]), int(coords_2d.shape[1])
    if prepared:
        assert coords_2d.dtype in _DTYPES and coords_2d_istd.dtype == coords_2d.dtype == coords_3d.dtype
        x2d, istd, x3d = coords_2d, coords_2d_istd, coords_3d
    else:
        dt = coords_2d.dtype if coords_2d.dtype in _DTYPES else torch.float32
        prep = lambda t: t.detach() if (t.dtype == dt and t.device == dev) else t.detach().to(device=dev, dtype=dt)
        x2d, istd, x3d = prep(coords_2d), prep(coords_2d_istd), prep(coords_3d)
    assert x2d.shape == (B, P, 2) and istd.shape == (B, P, 2) and x3d.shape == (B, P, 3)
    conv = lambda t, dtype, *shape: t.detach().to(device=dev, dtype=dtype).reshape(*shape).contiguous() if t is not None else None
    cam, ur, vr = conv(cam_mats, torch.float32, -1, 3, 3), conv(u_range, torch.float32, -1, 2), conv(v_range, torch.float32, -1, 2)
    keep = dict(x2d=x2d, istd=istd, x3d=x3d, cam_mats=cam, u_range=ur, v_range=vr, ransac_thr=conv(ransac_thr, torch.float32, -1),
                init_pose=conv(init_pose, torch.float64, -1, 4))
    common = dict(x2d=x2d.data_ptr(), x2d_strides=_strides(x2d), istd=istd.data_ptr(), istd_strides=_strides(istd), x3d=x3d.data_ptr(),
                  x3d_strides=_strides(x3d), in_dtype=_DTYPES[x2d.dtype], cam_mats=cam.data_ptr(), cam_batch=cam.shape[0])
    if ur is not None:
        assert ur.shape[0] == vr.shape[0]
        common.update(u_range=ur.data_ptr(), v_range=vr.data_ptr(), range_batch=ur.shape[0])
    return dev, B, P, common, keep


def _outputs(dev, B, P, with_diag, out=None, mask=None):
    """(valid u8 (B,), pose f32 (B,4), cov f32 (B,4,4), tr f32 (B,), mask u8 (B,P), diag f32 (B,4) | None) and the same as arguments under
    the header's names.  New tensors, or the valid / pose / cov / tr of `out` and the caller's `mask` buffer."""
    f32 = dict(device=dev, dtype=torch.float32)
    if out is None:
        valid, pose, cov, tr = torch.empty(B, device=dev, dtype=torch.uint8), torch.empty(B, 4, **f32), torch.empty(B, 4, 4, **f32), torch.empty(B, **f32)
    else:                                       # e.g. the typed views of parallel.PackedResults
        valid, pose, cov, tr = out.valid, out.pose, out.cov, out.tr
    if mask is None:
        mask = torch.empty(B, P, device=dev, dtype=torch.uint8)
    assert mask.shape == (B, P) and mask.dtype == torch.uint8 and mask.is_contiguous()
    diag = torch.empty(B, 4, **f32) if with_diag else None
    return (valid, pose, cov, tr, mask, diag), dict(valid=valid.data_ptr(), pose=pose.data_ptr(), cov=cov.data_ptr(), tr_radius=tr.data_ptr(),
                                                    inlier_mask=mask.data_ptr(), diag=_lib.ptr(diag))


def _init_buffers(dev, B, P):
    """What the initialiser hands to the LM launch: (init_pose f64 (B,4) [yaw0, t], init_mask u8 (B,P), init_valid u8 (B,))."""
    return (torch.empty(B, 4, device=dev, dtype=torch.float64), torch.empty(B, P, device=dev, dtype=torch.uint8),
            torch.empty(B, device=dev, dtype=torch.uint8))


def pnp_uncert_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=0.5,
                      epnp_istd_thres=1.0, epnp_ransac_thres=None, inlier_opt_only=False,
                      init_pose=None, flags=0, with_diag=False):
    """Launch the fused kernel on CUDA(HIP) tensors; returns raw device outputs
    (valid u8 (B,), pose f32 (B,4), cov f32 (B,4,4), tr f32 (B,), mask u8 (B,P), diag f32 (B,4)|None)."""
    lib = _lib.load()
    dev, B, P, common, keep = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres, init_pose,
                                      no_gpu='monorun_amd PnP runs on an MI355X only: inputs must be on a HIP device (there is no CPU fallback)')
    outs, out_args = _outputs(dev, B, P, with_diag)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_pnp_uncert_batched', common, ransac_thr=_lib.ptr(keep['ransac_thr']), init_pose=_lib.ptr(keep['init_pose']), B=B, P=P,
                      z_min=float(z_min), istd_thres=float(epnp_istd_thres), inlier_opt_only=int(bool(inlier_opt_only)), flags=int(flags),
                      **out_args, stream=torch.cuda.current_stream(dev).cuda_stream)
    return outs


def epnp_ransac_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, epnp_istd_thres=1.0, epnp_ransac_thres=None, flags=0,
                       max_iters=30, with_diag=False, debug_hypotheses=False, first_round=None):
    """The reference's own initialiser on the GPU (``mr_epnp_ransac_batched``): cv2.solvePnPRansac(..., iterationsCount=30,
    flags=SOLVEPNP_EPNP) on the istd candidates of every object (plain EPnP without thresholds), pnp_uncert_cpu.py:33-68.
    Returns (init_pose f64 (B,4) [yaw0, t], init_mask u8 (B,P), init_valid u8 (B,), diag f32 (B,4)|None, hypotheses f64 (B,30,12)|None)."""
    lib = _lib.load()
    dev, B, P, common, keep = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, ransac_thr=epnp_ransac_thres,
                                      no_gpu='monorun_amd EPnP/RANSAC runs on an MI355X only (no CPU fallback)')
    init_pose, init_mask, init_valid = _init_buffers(dev, B, P)
    diag = torch.empty(B, 4, device=dev, dtype=torch.float32) if with_diag else None
    hyp = torch.zeros(B, 30, 12, device=dev, dtype=torch.float64) if debug_hypotheses else None
    if B > 0:
        with torch.cuda.device(dev):
            # the launches of the call hand their intermediate results over in a workspace: from torch's caching allocator, on the
            # stream the launches go to (the block returns to the allocator when `work` dies; stream order keeps that safe)
            work = torch.empty(int(lib.mr_epnp_workspace_bytes(B, P)), device=dev, dtype=torch.uint8)
            _lib.call('mr_epnp_ransac_batched', common, ransac_thr=_lib.ptr(keep['ransac_thr']), B=B, P=P, istd_thres=float(epnp_istd_thres),
                      flags=_first_round_flags(flags, first_round), max_iters=int(max_iters), init_pose=init_pose.data_ptr(),
                      init_mask=init_mask.data_ptr(), init_valid=init_valid.data_ptr(), diag=_lib.ptr(diag), debug_hypotheses=_lib.ptr(hyp),
                      workspace=work.data_ptr(), workspace_bytes=work.numel(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return init_pose, init_mask, init_valid, diag, hyp


def pnp_uncert_from_init_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, init_pose, init_mask, init_valid,
                                z_min=0.5, inlier_opt_only=False, flags=0, with_diag=False):
    """LM + covariance from an external initialiser's (init_pose f64 (B,4), init_mask u8 (B,P), init_valid u8 (B,))
    (``mr_pnp_uncert_from_init_batched``).  Returns what ``pnp_uncert_device`` returns."""
    lib = _lib.load()
    dev, B, P, common, keep = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, init_pose=init_pose)
    im = init_mask.detach().to(device=dev, dtype=torch.uint8).contiguous()
    iv = init_valid.detach().to(device=dev, dtype=torch.uint8).contiguous()
    outs, out_args = _outputs(dev, B, P, with_diag)
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_pnp_uncert_from_init_batched', common, init_pose=keep['init_pose'].data_ptr(), init_mask=im.data_ptr(),
                      init_valid=iv.data_ptr(), B=B, P=P, z_min=float(z_min), inlier_opt_only=int(bool(inlier_opt_only)), flags=int(flags),
                      **out_args, stream=torch.cuda.current_stream(dev).cuda_stream)
    return outs


def pnp_uncert_epnp_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=0.5, epnp_istd_thres=1.0,
                           epnp_ransac_thres=None, inlier_opt_only=False, flags=0, max_iters=30, with_diag=False, first_round=None):
    """The reference's flow in one call: ``epnp_ransac_device`` with MR_EPNP_DEFER_REFIT, then ``mr_pnp_uncert_from_epnp_grouped`` — the LM +
    covariance launch that also runs the initialiser's last step (the re-fit's pose candidates) on the tile it loads anyway.  Same results,
    bit for bit, as ``epnp_ransac_device`` followed by ``pnp_uncert_from_init_device``; one launch and one pass over the correspondences
    less.  Returns (valid, pose, cov, tr, mask, diag|None, init_pose f64 (B,4), init_valid u8 (B,))."""
    lib = _lib.load()
    dev, B, P, common, keep = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres,
                                      no_gpu='monorun_amd EPnP/RANSAC runs on an MI355X only (no CPU fallback)')
    init_pose, init_mask, init_valid = _init_buffers(dev, B, P)
    init_args = dict(init_pose=init_pose.data_ptr(), init_mask=init_mask.data_ptr(), init_valid=init_valid.data_ptr())
    outs, out_args = _outputs(dev, B, P, with_diag)
    if B > 0:
        fused = 'mr_pnp_uncert_from_epnp_grouped'
        lm = dict(common, **init_args, **out_args)
        tables = {k: (ctypes.c_void_p * 1)(lm[k]) for k in _lib.table_args(fused) if k in lm}          # a launch set of one call
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            work = torch.empty(int(lib.mr_epnp_workspace_bytes(B, P)), device=dev, dtype=torch.uint8)     # (stream order keeps its reuse safe)
            work_args = dict(workspace=work.data_ptr(), workspace_bytes=work.numel())
            _lib.call('mr_epnp_ransac_batched', common, ransac_thr=_lib.ptr(keep['ransac_thr']), B=B, P=P, istd_thres=float(epnp_istd_thres),
                      flags=_first_round_flags(int(flags) & _INIT_FLAGS, first_round) | _lib.MR_EPNP_DEFER_REFIT, max_iters=int(max_iters),
                      **init_args, diag=None, debug_hypotheses=None, **work_args, stream=st)
            _lib.call(fused, common, ncalls=1, **tables, epnp_diag=None, B=B, P=P, z_min=float(z_min), inlier_opt_only=int(bool(inlier_opt_only)),
                      flags=int(flags), cov_calib_logscale=None, cov_corr_sd=0.0, cov_calib=None, **work_args, stream=st)
    return outs + (init_pose, init_valid)


def cov_symeig_rule_device(valid_u8, cov, with_eigs=False):
    """The reference's eigenvalue rule (pnp_uncert.py:77-85) applied IN PLACE to (valid u8 (B,), cov f32 (B,4,4)):
    objects with lambda_min(h) <= max(1e-6 lambda_max(h), 0) become invalid and get cov = I (``mr_cov_symeig_rule``)."""
    B = int(valid_u8.shape[0])
    assert valid_u8.dtype == torch.uint8 and cov.dtype == torch.float32 and cov.is_contiguous() and valid_u8.is_contiguous()
    lam = torch.empty(B, 2, device=cov.device, dtype=torch.float32) if with_eigs else None
    if B > 0:
        with torch.cuda.device(cov.device):
            _lib.call('mr_cov_symeig_rule', valid=valid_u8.data_ptr(), cov=cov.data_ptr(), B=B, eig_min_max=_lib.ptr(lam),
                      stream=torch.cuda.current_stream(cov.device).cuda_stream)
    return lam


class PnPLaunch:
    """A prepared launch of the fused kernel over device-resident inputs with preallocated outputs:
    every ctypes argument is built once, ``run()`` only enqueues the kernel on the current stream.
    Used where the same shapes recur (bench.py, sharded serving)."""

    def __init__(self, coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=0.5,
                 epnp_istd_thres=0.6, epnp_ransac_thres=None, inlier_opt_only=True, init_pose=None, flags=0,
                 out=None, with_diag=False, mask=None):
        self.lib = _lib.load()
        self.dev, B, P, common, self.keep = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres, init_pose,
                                                    no_gpu='PnPLaunch needs HIP device tensors (no CPU fallback)', prepared=True)
        (self.valid, self.pose, self.cov, self.tr, self.mask, self.diag), out_args = _outputs(self.dev, B, P, with_diag, out, mask)
        self.B = B
        self.named = dict(common, ransac_thr=_lib.ptr(self.keep['ransac_thr']), init_pose=_lib.ptr(self.keep['init_pose']), B=B, P=P, z_min=float(z_min),
                          istd_thres=float(epnp_istd_thres), inlier_opt_only=int(bool(inlier_opt_only)), flags=int(flags), **out_args)
        self.args = _lib.pack('mr_pnp_uncert_batched', self.named)

    def run(self, stream=None):
        if self.B == 0:
            return
        st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
        if torch.cuda.current_device() != self.dev.index:        # the library launches on the CURRENT HIP device
            with torch.cuda.device(self.dev):
                code = self.lib.mr_pnp_uncert_batched(*self.args, st)
        else:
            code = self.lib.mr_pnp_uncert_batched(*self.args, st)
        if code:
            _lib.check(code)


class PnPEpnpLaunch:
    """A prepared launch of the REFERENCE's flow over device-resident inputs: its initialiser (``mr_epnp_ransac_batched``: the
    launches of csrc/epnp_stages.inc, pnp_uncert_cpu.py:33-68) followed by the LM + covariance launch
    (``mr_pnp_uncert_from_init_batched``) on the same stream.  Outputs, the initialiser's hand-over buffers and its workspace
    (``mr_epnp_workspace_bytes``: 12.0 MB per 1024 objects) are allocated once; ``run()`` only enqueues.  The stages are latency
    chains that leave most issue slots of the chip idle, so several of these launches in flight (``PnPPipeline.submit``)
    overlap almost for free."""

    def __init__(self, coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=0.5, epnp_istd_thres=0.6,
                 epnp_ransac_thres=None, inlier_opt_only=True, flags=0, max_iters=30, with_diag=False, first_round=None,
                 out=None, mask=None, work=None, fused=True, calib=None):
        """calib: None, or (logscale, sd, out) — a float32 device tensor of the four calibration log-scales (read when the launch RUNS), the
        distance-correction constant (0 = none) and a (B,4,4) float32 tensor that receives (s s^T) * cov * (sd / ||t||)^2, written by the LM
        launch's epilogue (fused form only; uncert_prop_pnp_optimizer.py:96-97, monorun_roi_head.py:530-534).
        fused (default): the initialiser stops before its last launch (MR_EPNP_DEFER_REFIT) and the LM launch runs the re-fit's pose
        candidates as its prologue (``mr_pnp_uncert_from_epnp_grouped``: one launch and one pass over the correspondences less; same
        results, bit for bit); False: the two entry points one after the other (``mr_epnp_ransac_batched``, then
        ``mr_pnp_uncert_from_init_batched``).
        out: an object with valid / pose / cov / tr tensors to write the results into (e.g. the typed views of
        parallel.PackedResults: the kernel then writes straight into the buffer a collective sends); mask: the (B,P) uint8 inlier-mask
        buffer; work: a uint8 workspace of at least mr_epnp_workspace_bytes(B, P) bytes that SEVERAL launches may share when they
        only ever run on one stream (stream order keeps that safe).  All three default to tensors of the launch's own."""
        self.lib = lib = _lib.load()
        self.dev, B, P, common, self.keep = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres,
                                                    no_gpu='PnPEpnpLaunch needs HIP device tensors (no CPU fallback)', prepared=True)
        dev = self.dev
        self.init_pose, self.init_mask, self.init_valid = _init_buffers(dev, B, P)
        self.init_diag = torch.empty(B, 4, device=dev, dtype=torch.float32) if with_diag else None
        need = int(lib.mr_epnp_workspace_bytes(B, P)) if B > 0 else 0
        self.work = work if work is not None else torch.empty(need, device=dev, dtype=torch.uint8)
        assert self.work.dtype == torch.uint8 and self.work.numel() >= need and self.work.data_ptr() % 256 == 0
        (self.valid, self.pose, self.cov, self.tr, self.mask, self.diag), out_args = _outputs(dev, B, P, with_diag, out, mask)
        self.B = B
        init_args = dict(init_pose=self.init_pose.data_ptr(), init_mask=self.init_mask.data_ptr(), init_valid=self.init_valid.data_ptr())
        # the arguments of the two entry points by the header's names, on top of the common ones: what a launch set reads of its members
        # (plain numbers and ctypes arrays: nothing in them refers to this object)
        self.named_init = dict(common, ransac_thr=_lib.ptr(self.keep['ransac_thr']), B=B, P=P, istd_thres=float(epnp_istd_thres),
                               flags=_first_round_flags(int(flags) & _INIT_FLAGS, first_round), max_iters=int(max_iters), **init_args,
                               diag=_lib.ptr(self.init_diag), debug_hypotheses=None, workspace=self.work.data_ptr(), workspace_bytes=self.work.numel())
        self.named_lm = dict(common, **init_args, B=B, P=P, z_min=float(z_min), inlier_opt_only=int(bool(inlier_opt_only)), flags=int(flags), **out_args)
        self.args_init = _lib.pack('mr_epnp_ransac_batched', self.named_init)
        self.args_lm = _lib.pack('mr_pnp_uncert_from_init_batched', self.named_lm)
        self.calib = calib
        if calib is not None:
            ls, _, co = calib
            if not fused:
                raise ValueError('calib needs the fused form (the LM launch that carries the re-fit writes it)')
            assert ls.dtype == torch.float32 and ls.numel() == 4 and ls.device == dev and co.dtype == torch.float32 and co.is_contiguous() and co.numel() == B * 16
        self.fused = bool(fused)
        if self.fused:
            # the launch set of this one call.  It keeps argument lists (raw pointers into tensors THIS object owns), not this object: no
            # reference cycle, so the workspace / outputs / masks (~12.0 MB per 1024 objects) are freed by refcount when the launch is dropped
            # — a serving loop that builds launches per request does not wait for the cyclic GC
            self._single = PnPEpnpGroupLaunch([self], work=self.work, lm='fused')
            self._single.members = ()

    def run(self, stream=None):
        if self.B == 0:
            return
        if self.fused:
            return self._single.run(stream)
        st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
        with torch.cuda.device(self.dev):                 # the library launches on the CURRENT HIP device
            code = self.lib.mr_epnp_ransac_batched(*self.args_init, st)
            if not code:
                code = self.lib.mr_pnp_uncert_from_init_batched(*self.args_lm, st)
        if code:
            _lib.check(code)


# what the members of a launch set must agree in, by argument name: (equal values, pointers given or left out together), for the
# initialiser (mr_epnp_ransac_batched) and for the LM launch (mr_pnp_uncert_from_init_batched)
_SET_INIT = (('x2d_strides', 'istd_strides', 'x3d_strides', 'in_dtype', 'cam_batch', 'B', 'P', 'istd_thres', 'flags', 'max_iters'), ('ransac_thr', 'diag'))
_SET_LM = (('range_batch', 'z_min', 'inlier_opt_only', 'flags'), ('diag',))


def _require_agreement(members, rule, what):
    """ValueError unless the named arguments of every member agree with the first's under `rule` (_SET_INIT / _SET_LM)."""
    equal, together = rule
    val = lambda v: tuple(v) if isinstance(v, ctypes.Array) else v
    for m in members[1:]:
        if any(val(m[k]) != val(members[0][k]) for k in equal) or any((m[k] is None) != (members[0][k] is None) for k in together):
            raise ValueError(f'the members of a group must share {what}')


def _tables(fn, members, **per_member):
    """{name: (void *)[n] of the members' pointers} for every argument `fn` declares as a per-call pointer table; the pointers of a
    name come from `per_member` (a list) where it is given, else from the members' named arguments."""
    n = len(members)
    return {k: (ctypes.c_void_p * n)(*(per_member[k] if k in per_member else [m[k] for m in members])) for k in _lib.table_args(fn)}


class PnPEpnpGroupLaunch:
    """Up to eight prepared ``PnPEpnpLaunch`` objects of the same shape whose initialisers run as ONE launch set
    (``mr_epnp_ransac_grouped``: every launch of csrc/epnp_stages.inc carries the objects of all members), followed by each
    member's own LM + covariance launch, all on the stream ``run`` is given.  Members keep their inputs and outputs; results are
    bit-identical to running them one by one.  Why: HIP runs the launches of at most four streams side by side and the
    initialiser's stages are latency chains that fill a fraction of the chip, so a ``PnPPipeline`` of depth 4 that is fed groups
    of two keeps EIGHT calls' stages in flight (measured on MI355X, reference flow, 1024-object calls: DESIGN.md section 3)."""

    def __init__(self, launches, work=None, lm='fused'):
        """lm: how the members' LM + covariance launches are issued behind the set's initialiser — 'fused' (default): ONE launch over the
        objects of all members that also carries the initialiser's last step, the re-fit's pose candidates (MR_EPNP_DEFER_REFIT +
        ``mr_pnp_uncert_from_epnp_grouped``: one launch and one pass over the correspondences less); 'grouped': ONE launch over the
        objects of all members behind the complete initialiser (``mr_pnp_uncert_from_init_grouped``: the set pays its slowest object
        once); 'side_by_side': one launch per
        member, the second and later ones with MR_ANY_ORDER; 'serial': one per member in stream order.  Same results.
        work: a uint8 workspace of at least mr_epnp_workspace_bytes(len(launches) * B, P) bytes (shared between groups that only
        ever run on one stream), or None to allocate one."""
        self.members = list(launches)
        n = len(self.members)
        if not 1 <= n <= 8:
            raise ValueError('PnPEpnpGroupLaunch takes 1 to 8 launches')
        f = self.members[0]
        self.lib, self.dev, self.B = f.lib, f.dev, f.B
        inits, lms = [m.named_init for m in self.members], [m.named_lm for m in self.members]
        what = 'shape, strides, dtype, camera batching, thresholds and flags'
        if any(m.dev != f.dev for m in self.members):
            raise ValueError(f'the members of a group must share {what}')
        _require_agreement(inits, _SET_INIT, what)
        need = int(self.lib.mr_epnp_workspace_bytes(n * f.B, inits[0]['P'])) if f.B > 0 else 0
        self.work = work if work is not None else torch.empty(need, device=f.dev, dtype=torch.uint8)
        assert self.work.dtype == torch.uint8 and self.work.numel() >= need and self.work.data_ptr() % 256 == 0
        if lm not in ('fused', 'grouped', 'side_by_side', 'serial'):
            raise ValueError("lm must be 'fused', 'grouped', 'side_by_side' or 'serial'")
        work_args = dict(workspace=self.work.data_ptr(), workspace_bytes=self.work.numel())
        self.args = _lib.pack('mr_epnp_ransac_grouped', inits[0], ncalls=n, **_tables('mr_epnp_ransac_grouped', inits),
                              flags=inits[0]['flags'] | (_lib.MR_EPNP_DEFER_REFIT if lm == 'fused' else 0), **work_args)
        _require_agreement(lms, _SET_LM, 'range batching, z_min, inlier_opt_only and flags')
        self.lm = lm
        cal = [getattr(m, 'calib', None) for m in self.members]
        if any(c is not None for c in cal) and (any(c is None for c in cal) or any(c[0].data_ptr() != cal[0][0].data_ptr() or c[1] != cal[0][1] for c in cal)):
            raise ValueError('the members of a group must share the calibration (log-scale tensor and distance constant), or have none')
        if cal[0] is not None and lm != 'fused':
            raise ValueError("calibrated covariances are written by the 'fused' form")
        # the tables of the LM launch over the set, with the re-fit in it (the one behind the complete initialiser takes a part of them)
        tables = _tables('mr_pnp_uncert_from_epnp_grouped', lms, epnp_diag=[i['diag'] for i in inits],
                         cov_calib=[c[2].data_ptr() if c is not None else None for c in cal])
        if cal[0] is None:
            tables['cov_calib'] = None
        self.args_lm = _lib.pack('mr_pnp_uncert_from_init_grouped', dict(lms[0], **tables), ncalls=n)
        self.args_fused = _lib.pack('mr_pnp_uncert_from_epnp_grouped', lms[0], ncalls=n, **tables, cov_calib_logscale=cal[0][0].data_ptr() if cal[0] is not None else None,
                                    cov_corr_sd=float(cal[0][1]) if cal[0] is not None else 0.0, **work_args)
        # 'side_by_side': the members' own LM launches with MR_ANY_ORDER in their flags
        self._lm_any = [_lib.pack('mr_pnp_uncert_from_init_batched', l, flags=l['flags'] | _lib.MR_ANY_ORDER) for l in lms] if lm == 'side_by_side' else None

    def run(self, stream=None):
        if self.B == 0:
            return
        st = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
        with torch.cuda.device(self.dev):
            code = self.lib.mr_epnp_ransac_grouped(*self.args, st)
            if self.lm == 'fused':
                if not code:
                    code = self.lib.mr_pnp_uncert_from_epnp_grouped(*self.args_fused, st)
                if code:
                    _lib.check(code)
                return
            if not code and self.lm == 'grouped' and len(self.members) > 1:
                code = self.lib.mr_pnp_uncert_from_init_grouped(*self.args_lm, st)
                if code:
                    _lib.check(code)
                return
            for k, m in enumerate(self.members):
                if code:
                    break
                # the first call's LM launch waits for the set's initialiser launches (stream order); the others carry MR_ANY_ORDER:
                # they start as soon as the one in front of them has started, i.e. the set's LM launches run side by side instead
                # of each waiting for the slowest object of the one before
                code = self.lib.mr_pnp_uncert_from_init_batched(*(m.args_lm if (k == 0 or self.lm != 'side_by_side') else self._lm_any[k]), st)
        if code:
            _lib.check(code)


class PnPPipeline:
    """Several prepared launches in flight: ``submit`` issues them round-robin on ``depth`` internal HIP streams.

    Why: one launch of B = 1024 objects lasts as long as its slowest object (an object with 17 LM iterations keeps a handful
    of SIMDs busy for ~50 us while the other 1000 objects finished after ~35 us), and launches on ONE stream serialise, so a
    single stream pays that tail on every step.  Launches on different streams overlap: the next batches fill the SIMDs the
    tail leaves idle.  Every launch is still one full fused kernel over its own batch with its own output buffers; results
    are bit-identical to the single-stream ones (objects are independent; nothing is shared between launches).

        pipe = PnPPipeline(device, depth=4)
        ev = pipe.submit(launch)            # enqueue; `ev` completes when launch.valid / pose / cov / mask are written
        torch.cuda.current_stream().wait_event(ev)      # where (and when) a consumer stream needs them
        pipe.drain()                        # or: host-wait for everything submitted so far

    A launch object owns its output buffers, so the SAME PnPLaunch must not be submitted again before its previous run has
    completed unless it lands on the same internal stream (``slot`` pins a launch to a stream: give each buffer set a fixed
    slot and re-submissions are stream-ordered).  ``after`` = an event the inputs depend on (produced on another stream)."""

    def __init__(self, device, depth=4, record_events=True, avoid=(), verify=True):
        """depth: launches in flight asked for.  HIP maps a process's streams onto a few hardware queues (4 on this stack, the
        default stream's included) and two streams on one queue serialise — which of torch's pool streams collide is an internal
        of the runtime (on MI355X / ROCm 7.2 the first four pool streams land on three queues: 23 instead of 34 M solves/s).
        With verify=True the constructor therefore MEASURES it: candidates are taken from the pool and kept only if a 40 us
        one-wave spin kernel (mr_spin) on them runs side by side with one on every stream already kept — and on every stream in
        `avoid` (e.g. the side stream of parallel.RcclAllGather).  ``self.depth`` is the number of streams found (<= depth)."""
        self.dev = torch.device(device)
        if self.dev.type != 'cuda':
            raise RuntimeError('PnPPipeline needs a HIP device (no CPU fallback)')
        want = max(1, int(depth))
        self.overlap_test = None
        if verify and want > 1:
            self.streams, self.overlap_test = self._pick_streams(want, list(avoid))
        else:
            self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(want)]
        self.depth = len(self.streams)
        self.handles = [s.cuda_stream for s in self.streams]
        self.record_events = record_events
        self._next = 0

    def _pick_streams(self, want, avoid):
        import time
        US = 40

        def wall(a, b):
            best = 1e9
            for _ in range(3):
                a.synchronize(); b.synchronize()
                t0 = time.perf_counter()
                _lib.call('mr_spin', microseconds=US, stream=a.cuda_stream)
                _lib.call('mr_spin', microseconds=US, stream=b.cuda_stream)
                a.synchronize(); b.synchronize()
                best = min(best, time.perf_counter() - t0)
            return best * 1e6
        with torch.cuda.device(self.dev):
            torch.cuda.synchronize(self.dev)
            first = torch.cuda.Stream(device=self.dev)
            serial = wall(first, first)                      # two spins on ONE stream: what a collision looks like
            kept, tested = [first], 0
            if any(wall(first, a) > serial - 0.5 * US for a in avoid):
                kept = []
            for _ in range(8 * want + 8):
                if len(kept) >= want:
                    break
                c = torch.cuda.Stream(device=self.dev)
                tested += 1
                if any(c.cuda_stream == k.cuda_stream for k in kept):
                    continue
                if all(wall(c, k) < serial - 0.5 * US for k in kept + avoid):      # side by side: about one spin shorter than in series
                    kept.append(c)
            if not kept:
                kept = [first]
            torch.cuda.synchronize(self.dev)
        return kept, {'asked': want, 'found': len(kept), 'candidates_tested': tested + 1, 'serial_pair_us': serial}

    def flags_for(self, B, P=784):
        """The MR_WAVES bits for launches of B objects x P points issued through this pipeline.  The library chooses the number of
        wavefronts per object from ONE launch's size (4 up to B = 2048, 2 beyond: more waves shorten an object's latency chain,
        fewer cost fewer instructions per object); with `depth` launches in flight the chip holds depth x B objects, so the same
        rule is applied to that number (measured on MI355X, 1024-object launches, depth 4: 34 instead of 30 M solves/s)."""
        with torch.cuda.device(self.dev):
            w = int(_lib.load().mr_pick_waves(int(B) * self.depth, int(P)))       # the library's own rule (device properties included)
        if w < 0:
            _lib.check(w)
        return w << _lib.MR_WAVES_SHIFT

    def submit(self, launch, slot=None, after=None):
        k = (self._next if slot is None else int(slot)) % self.depth
        self._next += 1
        s = self.streams[k]
        if after is not None:
            s.wait_event(after)
        launch.run(self.handles[k])
        if not self.record_events:
            return None
        ev = getattr(launch, '_done_event', None)
        if ev is None:                                # created once per launch object (per output-buffer set)
            ev = launch._done_event = torch.cuda.Event()
        ev.record(s)
        return ev

    def drain(self):
        for s in self.streams:
            s.synchronize()


def pnp6_refine_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, inlier_mask_u8, pose4, valid4_u8, z_min=0.5,
                       flags=0, with_diag=False):
    """Second launch of the 6-DoF mode (``mr_pnp6_refine_batched``): 6-DoF LM from the 4-DoF result on its inlier set.
    Returns (valid u8 (B,), pose6 f32 (B,6) [rx,ry,rz,tx,ty,tz], cov6 f32 (B,6,6), diag f32 (B,2)|None); diag = [LM passes, exit reason as
    MR_DIAG_WHY].  flags: only the MR_LM_MAXIT bits are read.
    An object that never starts (valid4 == 0, or valid4 != 0 with an empty mask) is invalid with cov6 = identity and diag = (0, 8)
    ("initialiser failed"); its pose6 is zero when valid4 == 0 and the start pose (0, yaw, 0, t) otherwise.  A non-finite first
    evaluation (NaN / Inf in an inlier's data or in pose4) returns the start pose too: invalid, cov6 = identity, diag = (0, 7).  Fewer than
    three inliers never give a covariance (J^T J is singular): the LM's pose, invalid, cov6 = identity."""
    lib = _lib.load()
    dev, B, P, common, _ = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range)
    f32 = dict(device=dev, dtype=torch.float32)
    mask, pose4, valid4 = inlier_mask_u8.contiguous(), pose4.contiguous(), valid4_u8.contiguous()
    valid = torch.empty(B, device=dev, dtype=torch.uint8)
    pose6 = torch.empty(B, 6, **f32)
    cov6 = torch.empty(B, 6, 6, **f32)
    diag = torch.empty(B, 2, **f32) if with_diag else None
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_pnp6_refine_batched', common, inlier_mask=mask.data_ptr(), pose4=pose4.data_ptr(), valid4=valid4.data_ptr(), B=B, P=P,
                      z_min=float(z_min), flags=int(flags), valid=valid.data_ptr(), pose6=pose6.data_ptr(), cov6=cov6.data_ptr(),
                      diag=_lib.ptr(diag), stream=torch.cuda.current_stream(dev).cuda_stream)
    return valid, pose6, cov6, diag


def exact_hessian_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, pose4, inlier_mask_u8, valid_u8, z_min=0.5,
                         with_hessian=False):
    """`forward_exact_hessian=True` on device tensors (hessian.py:5-64 + pnp_uncert.py:63-85 of the reference): the exact Hessian of
    the masked cost at pose4 (B,4) f32 and its inverse.  inlier_mask_u8 (B,P) u8 | None, valid_u8 (B,) u8 = the 4-DoF solve's flags.
    Returns (valid u8 (B,), cov f32 (B,4,4), hess f32 (B,4,4) | None)."""
    lib = _lib.load()
    dev, B, P, common, _ = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range)
    f32 = dict(device=dev, dtype=torch.float32)
    valid = valid_u8.detach().to(device=dev, dtype=torch.uint8).clone().contiguous()
    pose = pose4.detach().to(**f32).contiguous()
    mask = inlier_mask_u8.detach().to(device=dev, dtype=torch.uint8).contiguous() if inlier_mask_u8 is not None else None
    cov = torch.empty(B, 4, 4, **f32)
    hess = torch.empty(B, 4, 4, **f32) if with_hessian else None
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_pnp_exact_hessian_batched', common, pose=pose.data_ptr(), inlier_mask=_lib.ptr(mask), B=B, P=P, z_min=float(z_min),
                      valid=valid.data_ptr(), hess=_lib.ptr(hess), cov=cov.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return valid, cov, hess


def pnp_uncert_backward_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, pose4, inlier_mask_u8, valid_u8, grad_pose,
                               cov=None, grad_cov=None, z_min=0.5, lm_all_points=False, needs=(True, True, True), with_status=False, out=None):
    """Backward of the 4-DoF op (``mr_pnp_uncert_backward_batched``): gradients of a loss L(pose, cov) with respect to
    the correspondences at the pose4 (B,4) f32 / inlier_mask_u8 (B,P) u8 | None / valid_u8 (B,) u8 the forward returned.
    grad_pose (B,4) = dL/d[yaw, t] or None (zero); cov (B,4,4) = the returned covariance and grad_cov (B,4,4) = dL/dcov, both or None.
    lm_all_points: the LM refined every point (inlier_opt_only=False).  needs: which of (x2d, istd, x3d) to compute.
    out: the caller's (grad_x2d, grad_istd, grad_x3d) buffers to write instead of new ones (f32, contiguous, on the inputs' device; None where
    `needs` is False); every row of every buffer is written.
    Returns (grad_x2d f32 (B,P,2) | None, grad_istd f32 (B,P,2) | None, grad_x3d f32 (B,P,3) | None, status u8 (B,) | None)."""
    lib = _lib.load()
    dev, B, P, common, _ = _inputs(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range,
                                   no_gpu='monorun_amd PnP backward runs on an MI355X only (no CPU fallback)')
    if (cov is None) != (grad_cov is None):
        raise ValueError('cov and grad_cov go together')
    f32 = dict(device=dev, dtype=torch.float32)
    conv = lambda t, *shape: t.detach().to(**f32).reshape(*shape).contiguous() if t is not None else None
    pose, gp, c, gc = conv(pose4, B, 4), conv(grad_pose, B, 4), conv(cov, B, 16), conv(grad_cov, B, 16)
    mask = inlier_mask_u8.detach().to(device=dev, dtype=torch.uint8).contiguous() if inlier_mask_u8 is not None else None
    valid = valid_u8.detach().to(device=dev, dtype=torch.uint8).contiguous()
    if out is None:
        out = [torch.empty(B, P, ch, **f32) if n else None for n, ch in zip(needs, (2, 2, 3))]
    for t, n, ch in zip(out, needs, (2, 2, 3)):
        assert (t is None) == (not n) and (t is None or (t.shape == (B, P, ch) and t.dtype == torch.float32 and t.device == dev and t.is_contiguous()))
    g2, gw, g3 = out
    status = torch.empty(B, device=dev, dtype=torch.uint8) if with_status else None
    if B > 0:
        with torch.cuda.device(dev):
            _lib.call('mr_pnp_uncert_backward_batched', common, pose=pose.data_ptr(), inlier_mask=_lib.ptr(mask), valid=valid.data_ptr(),
                      lm_all_points=int(bool(lm_all_points)), grad_pose=_lib.ptr(gp), cov=_lib.ptr(c), grad_cov=_lib.ptr(gc), B=B, P=P,
                      z_min=float(z_min), grad_x2d=_lib.ptr(g2), grad_istd=_lib.ptr(gw), grad_x3d=_lib.ptr(g3), status=_lib.ptr(status),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
    return g2, gw, g3, status


def _pnp_uncert_forward(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min, epnp_istd_thres, epnp_ransac_thres,
                        inlier_opt_only, forward_exact_hessian, use_6dof, initialiser, cov_symeig_rule, epnp_first_round):
    """The forward launches of ``pnp_uncert``.  Returns (outputs, saved): the op's tuple, and for the 4-DoF path the device tensors the
    backward needs (x2d, istd, x3d as the kernels read them, pose f32 (B,4), mask u8 (B,P), valid u8 (B,), cov f32 (B,4,4)); None for 6-DoF."""
    with torch.no_grad():
        src_dev = coords_2d.device
        if src_dev.type != 'cuda':
            if not torch.cuda.is_available():
                raise RuntimeError('monorun_amd.ops.pnp_uncert needs an MI355X (HIP) device; no CPU fallback exists')
            dev = torch.device('cuda', torch.cuda.current_device())
            mv = lambda t: t.to(dev) if t is not None else None
            coords_2d, coords_2d_istd, coords_3d = mv(coords_2d), mv(coords_2d_istd), mv(coords_3d)
        if initialiser is None:
            initialiser = DEFAULT_INITIALISER
        if initialiser == 'epnp':
            valid, pose, cov, _, mask = pnp_uncert_epnp_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=z_min,
                                                               epnp_istd_thres=epnp_istd_thres, epnp_ransac_thres=epnp_ransac_thres,
                                                               inlier_opt_only=inlier_opt_only, first_round=epnp_first_round)[:5]
        elif initialiser == 'k0':
            valid, pose, cov, _, mask, _ = pnp_uncert_device(
                coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=z_min,
                epnp_istd_thres=epnp_istd_thres, epnp_ransac_thres=epnp_ransac_thres, inlier_opt_only=inlier_opt_only)
        else:
            raise ValueError(f"initialiser must be 'k0' or 'epnp', got {initialiser!r}")
        odt = coords_2d.dtype
        if use_6dof and cov_symeig_rule:
            raise ValueError('cov_symeig_rule tests the 4x4 covariance of [yaw, t] (pnp_uncert.py:77-85); it has no meaning for the 6x6 '
                             'covariance that use_6dof=True returns')
        if use_6dof:
            valid6, pose6, cov6, _ = pnp6_refine_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, mask, pose, valid, z_min=z_min)
            return ((valid & valid6).to(device=src_dev, dtype=torch.bool), pose6[:, :3].to(device=src_dev, dtype=odt),
                    pose6[:, 3:].to(device=src_dev, dtype=odt), cov6.to(device=src_dev, dtype=odt), mask.to(device=src_dev, dtype=torch.bool)), None
        if forward_exact_hessian:
            valid, cov, _ = exact_hessian_device(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, pose, mask, valid, z_min=z_min)
        if cov_symeig_rule:
            cov = cov.contiguous()
            cov_symeig_rule_device(valid, cov)
        ret_val = valid.to(device=src_dev, dtype=torch.bool)
        r_vec = pose[:, :1].to(device=src_dev, dtype=odt)
        t_vec = pose[:, 1:].to(device=src_dev, dtype=odt)
        pose_cov = cov.to(device=src_dev, dtype=odt)
        inlier_mask = mask.to(device=src_dev, dtype=torch.bool)
    return (ret_val, r_vec, t_vec, pose_cov, inlier_mask), (coords_2d, coords_2d_istd, coords_3d, pose, mask, valid, cov)


class _PnPUncertFunction(torch.autograd.Function):
    """``pnp_uncert(..., differentiable=True)``: the forward launches of the op unchanged; the backward is one launch of
    ``mr_pnp_uncert_backward_batched`` (implicit differentiation at the refined pose).  Differentiable in the three
    coordinate tensors; cam_mats, u_range, v_range and epnp_ransac_thres get None (as the reference's get_jacobians)."""

    @staticmethod
    def forward(ctx, coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres, kw):
        (ret_val, r_vec, t_vec, pose_cov, inlier_mask), saved = _pnp_uncert_forward(
            coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres=epnp_ransac_thres, **kw)
        ctx.save_for_backward(*saved)
        ctx.cam, ctx.ur, ctx.vr = cam_mats.detach(), u_range.detach(), v_range.detach()
        ctx.z_min, ctx.lm_all = kw['z_min'], not kw['inlier_opt_only']
        ctx.src = [(t.device, t.dtype) for t in (coords_2d, coords_2d_istd, coords_3d)]
        ctx.mark_non_differentiable(ret_val, inlier_mask)
        # r_vec / t_vec may be views of one pose buffer: hand out tensors of their own (same values)
        return ret_val, r_vec.clone(), t_vec.clone(), pose_cov, inlier_mask

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, _g_ret, g_r, g_t, g_cov, _g_mask):
        x2d, istd, x3d, pose, mask, valid, cov = ctx.saved_tensors
        needs = tuple(ctx.needs_input_grad[:3])
        if not any(needs) or (g_r is None and g_t is None and g_cov is None):
            return (None,) * 8
        B, dev = pose.shape[0], pose.device
        f32 = dict(device=dev, dtype=torch.float32)
        gp = torch.zeros(B, 4, **f32)
        if g_r is not None:
            gp[:, :1] = g_r.to(**f32)
        if g_t is not None:
            gp[:, 1:] = g_t.to(**f32)
        gc = g_cov.to(**f32) if g_cov is not None else None
        grads = pnp_uncert_backward_device(x2d, istd, x3d, ctx.cam, ctx.ur, ctx.vr, pose, mask, valid, gp, cov if gc is not None else None, gc,
                                           z_min=ctx.z_min, lm_all_points=ctx.lm_all, needs=needs)[:3]
        out = [g.to(device=d, dtype=t) if g is not None else None for g, (d, t) in zip(grads, ctx.src)]
        return tuple(out) + (None,) * 5


def pnp_uncert(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, z_min=0.5, epnp_istd_thres=1.0,
               epnp_ransac_thres=None, inlier_opt_only=False, forward_exact_hessian=False, use_6dof=False, initialiser=None, cov_symeig_rule=False,
               epnp_first_round=None, differentiable=False):
    """Functional form of the op on torch tensors (argument names and defaults: pnp_uncert.py:7-11 of the reference).

    coords_2d / coords_2d_istd (B,P,2), coords_3d (B,P,3), cam_mats (B|1,3,3), u_range / v_range (B|1,2),
    epnp_ransac_thres (B,) or None — any device; host tensors are staged through the GPU.
    forward_exact_hessian=True (no shipped config, e.g. configs/kitti_car.py:123 sets False; the reference's own exact Hessian no
    longer runs on torch >= 2): pose_cov = inverse of the exact Hessian of the masked cost (hessian.py:5-64) instead of
    inverse(J^T J) — a second launch (exact_hessian_device); ignored together with use_6dof=True (the 6-DoF covariance is the
    solver's J^T J).
    initialiser (not a reference keyword; default = DEFAULT_INITIALISER = 'epnp'): 'epnp' = the reference's own initialiser —
    cv2.solvePnPRansac(..., iterationsCount=30, flags=SOLVEPNP_EPNP), pnp_uncert_cpu.py:33-68 — as its own sequence of launches in front
    of the LM launch (the published algorithm as DESIGN.md §5 restates it: inlier sets, start pose and hence the returned pose are the
    reference flow's, up to what OpenCV's own build would do); 'k0' = the explicit FAST MODE: this repository's deterministic consensus
    initialiser inside the fused kernel (one launch, ~5 x the throughput, inlier sets that differ from the reference flow's on ~13 % of
    the objects).
    epnp_first_round (with initialiser='epnp'; not a reference keyword): how many of the 30 speculative RANSAC hypotheses are solved for
    every object before the replayed loop is consulted (default: the library's rule — 10 for calls or launch sets of fewer than 2048 objects,
    3 beyond —; the rest only where the loop wants them; 30 = one round, the setting
    for outlier-heavy candidate sets one call at a time).  Never changes a result.
    cov_symeig_rule (not a reference keyword): also apply, per object, the eigenvalue test of the reference's fallback branch
    (pnp_uncert.py:77-85: keep an object only if lambda_min(h) > max(1e-6 lambda_max(h), 0), else ret_val = False and pose_cov = I).
    Default False = this kernel's own rule (an object is dropped when h has no Cholesky factorisation), which is what the
    reference does whenever torch.inverse does not raise.
    use_6dof=False (every shipped config): returns (ret_val (B,) bool, r_vec (B,1) yaw, t_vec (B,3), pose_cov (B,4,4) covariance of
    [yaw, t], inlier_mask (B,P) bool) on the device and in the dtype of coords_2d — the reference's tuple.
    use_6dof=True: the flag the reference declares and never reads (pnp_uncert.py:11) made real — after the 4-DoF solve (mask,
    initial pose) a second launch refines all six pose parameters with the same residual and LM: r_vec becomes the (B,3)
    angle-axis vector, pose_cov the (B,6,6) covariance of [rx, ry, rz, tx, ty, tz] (solver Jacobian); ret_val additionally
    requires the 6-DoF solve to be usable.  Because the flag is dead in the reference, every shipped config keeps running
    the 4-DoF path.
    differentiable (not a reference keyword; default False): when True and a coordinate tensor requires grad, the op is a
    ``torch.autograd.Function`` — the same launches and bit-identical outputs, and r_vec / t_vec / pose_cov carry gradients to
    coords_2d, coords_2d_istd and coords_3d (the reference's documented backward, pnp_uncert.py:102-105, with the exact Hessian;
    DESIGN.md §10).  Not with use_6dof=True or forward_exact_hessian=True (ValueError).
    """
    if differentiable and (use_6dof or forward_exact_hessian):
        raise ValueError('differentiable=True covers the 4-DoF pose with the J^T J covariance: not use_6dof=True or forward_exact_hessian=True')
    kw = dict(z_min=z_min, epnp_istd_thres=epnp_istd_thres, inlier_opt_only=inlier_opt_only, forward_exact_hessian=forward_exact_hessian,
              use_6dof=use_6dof, initialiser=initialiser, cov_symeig_rule=cov_symeig_rule, epnp_first_round=epnp_first_round)
    if differentiable and torch.is_grad_enabled() and any(t.requires_grad for t in (coords_2d, coords_2d_istd, coords_3d)):
        return _PnPUncertFunction.apply(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres, kw)
    return _pnp_uncert_forward(coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres=epnp_ransac_thres, **kw)[0]


@PNP.register_module()
class PnPUncert(torch.nn.Module):

    def __init__(self, z_min=0.5, epnp_istd_thres=0.6, inlier_opt_only=True, coord_istd_normalize=False,
                 forward_exact_hessian=False, use_6dof=False, eps=1e-6, initialiser=None, epnp_first_round=None, cov_symeig_rule=False,
                 differentiable=False):
        """Module form (constructor keywords of the reference, pnp_uncert.py:93-99; no parameters, no buffers).
        epnp_istd_thres: a point is an istd inlier when both of its istd components reach this factor times the object's
        mean; inlier_opt_only: the LM refines on the inlier set only; coord_istd_normalize: divide the istd map by its
        per-object mean (clamped at eps) first.  initialiser ('k0' | 'epnp'), epnp_first_round, cov_symeig_rule (not reference
        keywords): see ``pnp_uncert``.  The reference's own config dict builds the REFERENCE's flow (initialiser='epnp', the default since
        round 5); ``initialiser='k0'`` selects the one-launch fast mode.  differentiable (not a reference keyword):
        gradients flow from yaw / t_vec / pose_cov to the coordinate maps (``pnp_uncert``; the istd normalisation stays in torch)."""
        super().__init__()
        if initialiser is None:
            initialiser = DEFAULT_INITIALISER
        if initialiser not in ('k0', 'epnp'):
            raise ValueError(f"initialiser must be 'k0' or 'epnp', got {initialiser!r}")
        if cov_symeig_rule and use_6dof:
            raise ValueError('cov_symeig_rule applies to the 4-DoF covariance only (use_6dof=True returns a 6x6 one)')
        if differentiable and (use_6dof or forward_exact_hessian):
            raise ValueError('differentiable=True covers the 4-DoF pose with the J^T J covariance: not use_6dof=True or forward_exact_hessian=True')
        self.differentiable = differentiable
        self.initialiser, self.epnp_first_round, self.cov_symeig_rule = initialiser, epnp_first_round, cov_symeig_rule
        self.z_min, self.epnp_istd_thres, self.inlier_opt_only = z_min, epnp_istd_thres, inlier_opt_only
        self.coord_istd_normalize, self.eps = coord_istd_normalize, eps
        self.forward_exact_hessian, self.use_6dof = forward_exact_hessian, use_6dof

    def forward(self, coords_2d, coords_2d_istd, coords_3d, cam_mats, u_range, v_range, epnp_ransac_thres=None):
        istd = coords_2d_istd
        if self.coord_istd_normalize:
            istd = istd / istd.mean(dim=(1, 2), keepdim=True).clamp(min=self.eps)
        return pnp_uncert(coords_2d, istd, coords_3d, cam_mats, u_range, v_range, z_min=self.z_min,
                          epnp_istd_thres=self.epnp_istd_thres, epnp_ransac_thres=epnp_ransac_thres,
                          inlier_opt_only=self.inlier_opt_only, forward_exact_hessian=self.forward_exact_hessian,
                          use_6dof=self.use_6dof, initialiser=self.initialiser, epnp_first_round=self.epnp_first_round,
                          cov_symeig_rule=self.cov_symeig_rule, differentiable=self.differentiable)
