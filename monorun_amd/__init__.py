"""monorun_amd — MI355X-native (gfx950 HIP) implementation of MonoRUn's uncertainty-aware PnP hot path.

Drop-in surface: ``monorun_amd.ops`` mirrors the reference's ``monorun.ops``
(build_pnp / PnPUncert / pnp_uncert / u2d_pnp_cpu / PNP).  Around it: ``pose_head`` (NOC-head decode, pose head mirror,
fused head -> pose launch, RoIAlign), ``noc_head`` (the NOC head's training decode, targets and loss), ``noc_targets`` (its dense LiDAR targets), ``noc_decoder`` (the NOC head's trunk, ``FCNNOCDecoder``), ``carafe`` (its fused CARAFE upsampler), ``roi_extractor`` (the multi-level RoI feature extractors in front of every head), ``rpn_head`` (the region proposal head, ``RPNHeadMod``, which produces the RoIs) over ``proposals`` (its fused proposal decode and the grouped axis-aligned NMS: ``nms``, ``batched_nms``, ``multiclass_nms``), ``bbox_head`` (the 2-D detection head, ``Shared2FCBBoxHead``, and its fused ``get_bboxes``), ``consumers`` (3-D box packing, rotated-BEV NMS, and ``result_3d_nms``: poses and scores to the class-grouped NMS result in one launch), ``roi_head`` (``MonoRUnRoIHead``: the reference's ``simple_test`` over all of these, a fast path of fused launches and the literal chain) and ``detector`` (``MonoRUnDetector``: image in, ``bbox_3d_results`` out), ``image_pipeline`` (pixels to the detector's inputs: flip, photometric distortion, normalise and pad in one launch, ``init_detector`` / ``inference_detector``), ``evaluation`` (KITTI evaluator and
wire format), ``parallel`` (object sharding, RCCL exchange), ``synthetic`` (seeded workloads).  See DESIGN.md and INTEGRATION.md.
"""
from . import _lib  # noqa: F401
from .ops import build_pnp, PnPUncert, pnp_uncert, u2d_pnp_cpu, PNP  # noqa: F401
from .ops.least_squares.pnp_uncert import PnPLaunch, PnPEpnpLaunch, PnPEpnpGroupLaunch, PnPPipeline, pnp_uncert_device  # noqa: F401
from .carafe import CARAFEPack, carafe_pack, carafe_pack_torch  # noqa: F401  (the plain op stays monorun_amd.carafe.carafe: its name is the module's)
from .noc_decoder import FCNNOCDecoder  # noqa: F401
from .roi_extractor import SingleRoIExtractor, SingleRoIExtractorMod, roi_extract, roi_extract_torch  # noqa: F401
from .proposals import nms, batched_nms, multiclass_nms  # noqa: F401
from .rpn_head import AnchorGenerator, RPNHeadMod  # noqa: F401
from .bbox_head import Shared2FCBBoxHead, bbox2roi, bbox2result  # noqa: F401
from .roi_head import MonoRUnRoIHead  # noqa: F401
from .detector import MonoRUnDetector  # noqa: F401
from .image_pipeline import (PhotoParams, draw_augmentation, flip_bboxes, inference_detector, init_detector, load_image,  # noqa: F401
                             prepare_batch, prepare_batch_torch, prepare_train_batch)

__version__ = '0.1.0'
