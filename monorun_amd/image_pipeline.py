"""From pixels to the detector's inputs: what the reference's data pipeline runs on CPU workers between
``mmcv.imread`` and the collated batch — ``RandomFlip3D`` of the image, the boxes and the ``coord_2d`` field, mmdet's
``PhotoMetricDistortion``, ``Normalize``, ``Pad3D`` (zeros for the image, ``padding_mode='edge'`` for ``coord_2d``) and collate's zero
padding to the batch's largest shape — and the reference's ``init_detector`` / ``inference_detector`` over it.  Neither mmcv nor mmdet nor
OpenCV is needed.

    prepare_batch(images, mean, std, ...) -> (img (N, 3, Hb, Wb), coord_2d (N, 2, Hb, Wb), img_metas)

Two paths over one definition (include/monorun_image.h states it operation by operation):

  fast      ``mr_image_prepare``: the uint8 images travel packed (3 bytes per pixel instead of 20), ONE HIP launch writes both outputs,
            every element once; no host synchronisation.  Runs for a CUDA device, uint8 images with 3 channels, within the caps.
  literal   :func:`prepare_batch_torch`: torch ops in the same operation order on any device; bit for bit the launch.

:func:`fast_path_reason` names what sends a call to the literal path, ``path='fast'`` raises it, ``last_path`` records what ran.

The colour conversions of the photometric chain are OpenCV's float32 formulas as this project restates them from the scalar code path;
OpenCV is not available where this was written, so they are this project's DEFINITION and are not pinned against ``cv2``
(tests/golden/make_golden_image_prepare.py records the fixture that would pin them).

The augmentation's parameters are explicit data (:class:`PhotoParams`, drawn by :func:`draw_augmentation` from a
``numpy.random.RandomState`` in mmdet's statement order), so a run is reproducible.  Stream compatibility with a particular mmdet
release's use of the global RNG is NOT claimed: mmdet 2.3 draws the flip by ``np.random.rand() < flip_ratio`` (what is done here), 2.7 by
``np.random.choice`` over the directions.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .pose_head import gen_coord_2d
from .proposals import host_to_device

MAX_IMAGES = 65535                      # MR_IMAGE_MAX_IMAGES
MAX_PIXELS = 2 ** 31 - 1                # MR_IMAGE_MAX_PIXELS
TABLE_WORDS = 16                        # MR_IMAGE_TABLE_WORDS
SW_BRIGHTNESS, SW_CONTRAST, SW_CONTRAST_FIRST, SW_SATURATION, SW_HUE, SW_HSV = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
FLT_EPSILON = float(np.finfo(np.float32).eps)

last_path = None                        # 'fast' or 'literal': what the latest prepare_batch ran


class PhotoParams:
    """One image's photometric parameters: mmdet's ``PhotoMetricDistortion`` with its coins already tossed.  ``None`` switches a step
    off.  ``contrast_mode`` 1 applies ``contrast_alpha`` before the HSV round trip, 0 after it.  ``permutation``: output channel c is the
    chain's channel ``permutation[c]`` (``img[..., perm]``).  ``hsv``: the BGR -> HSV -> BGR round trip, which mmdet runs whenever the
    transform runs (it is not the identity in float32); ``hsv=False`` with a saturation or hue step is an error.  An image that is not
    distorted at all takes ``photometric=None`` in :func:`prepare_batch`, not a ``PhotoParams``."""
    __slots__ = ('brightness_delta', 'contrast_mode', 'contrast_alpha', 'saturation_alpha', 'hue_delta', 'permutation', 'hsv')

    def __init__(self, brightness_delta=None, contrast_mode=0, contrast_alpha=None, saturation_alpha=None, hue_delta=None, permutation=None,
                 hsv=True):
        self.brightness_delta, self.contrast_mode, self.contrast_alpha = brightness_delta, int(contrast_mode), contrast_alpha
        self.saturation_alpha, self.hue_delta, self.hsv = saturation_alpha, hue_delta, bool(hsv)
        self.permutation = None if permutation is None else tuple(int(p) for p in permutation)

    def switches(self):
        sw = (SW_BRIGHTNESS if self.brightness_delta is not None else 0) | (SW_CONTRAST if self.contrast_alpha is not None else 0)
        sw |= (SW_CONTRAST_FIRST if self.contrast_mode == 1 else 0) | (SW_SATURATION if self.saturation_alpha is not None else 0)
        return sw | (SW_HUE if self.hue_delta is not None else 0) | (SW_HSV if self.hsv else 0)

    def as_tuple(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, PhotoParams) and self.as_tuple() == other.as_tuple()

    def __repr__(self):
        return 'PhotoParams(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in self.__slots__) + ')'


def draw_augmentation(rng, flip_ratio=0.5, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18):
    """One image's ``(flip, PhotoParams)`` from ``rng`` (a ``numpy.random.RandomState``), consumed in the statement order of mmdet's
    ``RandomFlip`` (2.3: ``rand() < flip_ratio``) and ``PhotoMetricDistortion.__call__``: the flip; the brightness coin and value; the
    mode; with mode 1 the contrast coin and value; the saturation coin and value; the hue coin and value; with mode 0 the contrast coin
    and value; the permutation coin and ``permutation(3)``.  A coin is ``randint(2)``, a value is drawn only when its coin shows 1."""
    flip = bool(rng.rand() < flip_ratio)
    p = PhotoParams()
    if rng.randint(2):
        p.brightness_delta = float(rng.uniform(-brightness_delta, brightness_delta))
    p.contrast_mode = int(rng.randint(2))
    if p.contrast_mode == 1:
        if rng.randint(2):
            p.contrast_alpha = float(rng.uniform(contrast_range[0], contrast_range[1]))
    if rng.randint(2):
        p.saturation_alpha = float(rng.uniform(saturation_range[0], saturation_range[1]))
    if rng.randint(2):
        p.hue_delta = float(rng.uniform(-hue_delta, hue_delta))
    if p.contrast_mode == 0:
        if rng.randint(2):
            p.contrast_alpha = float(rng.uniform(contrast_range[0], contrast_range[1]))
    if rng.randint(2):
        p.permutation = tuple(int(i) for i in rng.permutation(3))
    return flip, p


def flip_bboxes(bboxes, img_shape):
    """mmdet's horizontal ``bbox_flip``: ``x1' = w - x2``, ``x2' = w - x1`` for boxes (.., 4k), a tensor or an array; a copy."""
    assert bboxes.shape[-1] % 4 == 0
    w = img_shape[1]
    flipped = bboxes.clone() if isinstance(bboxes, torch.Tensor) else np.array(bboxes, copy=True)
    flipped[..., 0::4] = w - bboxes[..., 2::4]
    flipped[..., 2::4] = w - bboxes[..., 0::4]
    return flipped


def load_image(path):
    """``mmcv.imread``'s contract through PIL: the file as a uint8 (h, w, 3) array in B, G, R order."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


# ------------------------------------------------------------------------------------------------ the table of the launch
def _round_up(v, d):
    return -(-int(v) // d) * d


def _f32_bits(v):
    return int(np.array(0.0 if v is None else v, dtype=np.float32).view(np.int32))


def table_row(offset, h, w, stride, flip=False, photometric=None):
    """One image's row of the launch's table (include/monorun_image.h): MR_IMAGE_TABLE_WORDS int32 words."""
    row = np.zeros(TABLE_WORDS, dtype=np.int32)
    p = photometric
    perm = (0, 1, 2) if p is None or p.permutation is None else p.permutation
    if len(perm) != 3 or any(not 0 <= int(c) <= 3 for c in perm):
        raise ValueError(f'image_prepare: {perm!r} is not a permutation of the three channels')
    off = np.array([offset], dtype=np.int64).view(np.int32)
    row[0], row[1] = off[0], off[1]
    row[2:6] = np.array([h, w, stride, 1 if flip else 0], dtype=np.int64).astype(np.int32)
    row[6] = 0 if p is None else p.switches()
    row[7] = int(perm[0]) | int(perm[1]) << 2 | int(perm[2]) << 4
    if p is not None:
        row[8], row[9] = _f32_bits(p.brightness_delta), _f32_bits(p.contrast_alpha)
        row[10], row[11] = _f32_bits(p.saturation_alpha), _f32_bits(p.hue_delta)
    return row


def check_table(rows, src_bytes, size_divisor, batch_shape, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """The host checks of ``mr_image_prepare`` in Python, on host data alone: ``ValueError`` naming what the entry point would reject with
    MR_ERR_BAD_ARGUMENT, ``NotImplementedError`` for what is beyond its caps.  Nothing is launched."""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, TABLE_WORDS)
    d, (Hb, Wb) = int(size_divisor), (int(batch_shape[0]), int(batch_shape[1]))
    if d < 4 or d % 4:
        raise ValueError(f'image_prepare: size_divisor {d} is not a positive multiple of 4')
    if Hb < d or Wb < d or Hb % d or Wb % d:
        raise ValueError(f'image_prepare: the batch shape {(Hb, Wb)} is not a positive multiple of size_divisor {d}')
    if len(mean) != 3 or len(std) != 3 or not all(np.isfinite(float(m)) for m in mean) or not all(np.isfinite(float(s)) and float(s) > 0 for s in std):
        raise ValueError('image_prepare: mean and std are three finite numbers each, std positive')
    if len(rows) > MAX_IMAGES:
        raise NotImplementedError(f'image_prepare: {len(rows)} images, the launch takes {MAX_IMAGES}')
    if Hb * Wb > MAX_PIXELS:
        raise NotImplementedError(f'image_prepare: a batch shape of {Hb} x {Wb} is beyond 32-bit indexing')
    if int(src_bytes) < 0:
        raise ValueError('image_prepare: a negative buffer size')
    for n, r in enumerate(rows):
        off = int(r[:2].copy().view(np.int64)[0])
        h, w, stride, sw, p = int(r[2]), int(r[3]), int(r[4]), int(r[6]), int(r[7])
        if h < 1 or w < 1:
            raise ValueError(f'image_prepare: image {n} has the size {h} x {w}')
        if stride < 3 * w:
            raise ValueError(f'image_prepare: image {n} has a row stride of {stride} bytes, below 3 w = {3 * w}')
        if off < 0 or off > int(src_bytes) or (h - 1) * stride + 3 * w > int(src_bytes) - off:
            raise ValueError(f'image_prepare: image {n} (offset {off}, {h} rows of stride {stride}) leaves the buffer of {int(src_bytes)} bytes')
        if _round_up(h, d) > Hb or _round_up(w, d) > Wb:
            raise ValueError(f'image_prepare: image {n} pads to {(_round_up(h, d), _round_up(w, d))}, beyond the batch shape {(Hb, Wb)}')
        if sw & ~0x3f or (sw & (SW_SATURATION | SW_HUE) and not sw & SW_HSV):
            raise ValueError(f'image_prepare: image {n} has the switches {sw:#x}: saturation and hue need the HSV round trip')
        if p & ~0x3f or (1 << (p & 3) | 1 << (p >> 2 & 3) | 1 << (p >> 4 & 3)) != 7:
            raise ValueError(f'image_prepare: image {n} has a channel permutation that is not one of the six')
        if not np.all(np.isfinite(r[8:12].copy().view(np.float32))):
            raise ValueError(f'image_prepare: image {n} has a photometric parameter that is not finite')
    return rows


def image_prepare(src, rows, mean, std, to_rgb=True, size_divisor=32, batch_shape=None):
    """``mr_image_prepare`` on a packed device buffer: src (bytes,) uint8 on a CUDA device, rows (N, 16) int32 on the host
    (:func:`table_row`).  -> img (N, 3, Hb, Wb), coord_2d (N, 2, Hb, Wb).  ONE launch, no host synchronisation: the table reaches the
    device through pinned memory, in stream order."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, TABLE_WORDS))
    d = int(size_divisor)
    if batch_shape is None:
        batch_shape = (max((_round_up(r[2], d) for r in rows), default=d), max((_round_up(r[3], d) for r in rows), default=d))
    if not isinstance(src, torch.Tensor) or src.device.type != 'cuda' or src.dtype != torch.uint8 or not src.is_contiguous():
        raise TypeError('image_prepare: src is a contiguous uint8 tensor on a CUDA device')
    check_table(rows, src.numel(), d, batch_shape, mean, std)
    N, (Hb, Wb), dev = len(rows), (int(batch_shape[0]), int(batch_shape[1])), src.device
    img = torch.empty(N, 3, Hb, Wb, dtype=torch.float32, device=dev)
    coord = torch.empty(N, 2, Hb, Wb, dtype=torch.float32, device=dev)
    if N == 0:
        return img, coord
    table = torch.from_numpy(rows).pin_memory().to(dev, non_blocking=True)
    d3 = ctypes.c_double * 3
    with torch.cuda.device(dev):
        _lib.call('mr_image_prepare', src=src.data_ptr(), src_bytes=src.numel(), table=rows.ctypes.data, table_device=table.data_ptr(),
                  n_images=N, mean=d3(*[float(m) for m in mean]), std=d3(*[float(s) for s in std]), to_rgb=int(bool(to_rgb)),
                  size_divisor=d, batch_h=Hb, batch_w=Wb, img=img.data_ptr(), coord_2d=coord.data_ptr(),
                  stream=torch.cuda.current_stream(dev).cuda_stream)
    return img, coord


# ------------------------------------------------------------------------------------------------ the literal path
def photometric_torch(b, g, r, p):
    """The chain of include/monorun_image.h on fp32 tensors b, g, r: one torch op per stated operation (a Python scalar enters an op as
    its float32 value).  -> (b, g, r) before the channel permutation."""
    if p.brightness_delta is not None:
        b, g, r = b + p.brightness_delta, g + p.brightness_delta, r + p.brightness_delta
    if p.contrast_alpha is not None and p.contrast_mode == 1:
        b, g, r = b * p.contrast_alpha, g * p.contrast_alpha, r * p.contrast_alpha
    if p.hsv:
        V = torch.maximum(b, torch.maximum(g, r))
        d = V - torch.minimum(b, torch.minimum(g, r))
        S = d / (V.abs() + FLT_EPSILON)
        k = (60.0 / (d + FLT_EPSILON).double()).float()
        H = torch.where(V == r, (g - b) * k, torch.where(V == g, (b - r) * k + 120.0, (r - g) * k + 240.0))
        H = torch.where(H < 0, H + 360.0, H)
        if p.saturation_alpha is not None:
            S = S * p.saturation_alpha
        if p.hue_delta is not None:
            H = H + p.hue_delta
            H = torch.where(H > 360, H - 360.0, H)
            H = torch.where(H < 0, H + 360.0, H)
        hs = H * float(np.float32(6.0 / 360.0))
        fl = torch.floor(hs)
        f = hs - fl
        inside = (fl >= 0) & (fl <= 5)
        fl, f = torch.where(inside, fl, torch.zeros_like(fl)), torch.where(inside, f, torch.zeros_like(f))
        tab = torch.stack((V, V * (1.0 - S), V * (1.0 - S * f), V * (1.0 - S * (1.0 - f))))
        rows = torch.tensor([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
        if b.device.type == 'cuda':
            rows = rows.pin_memory().to(b.device, non_blocking=True)
        pick = rows[fl.long()]                                                        # (.., 3)
        grey = S == 0
        b, g, r = (torch.where(grey, V, tab.gather(0, pick[..., c][None])[0]) for c in range(3))
    if p.contrast_alpha is not None and p.contrast_mode != 1:
        b, g, r = b * p.contrast_alpha, g * p.contrast_alpha, r * p.contrast_alpha
    return b, g, r


def _as_hwc(image, device):
    t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f'prepare_batch: an image is (h, w, 3), not {tuple(t.shape)}')
    if t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError('prepare_batch: an empty image')
    if device.type == 'cuda' and t.device.type == 'cpu':
        return t.pin_memory().to(device, non_blocking=True)
    return t.to(device)


def prepare_batch_torch(images, mean, std, to_rgb=True, size_divisor=32, flips=None, photometric=None, device=None):
    """The literal path: ``(img, coord_2d)`` in torch ops on ``device``, in the operation order of include/monorun_image.h."""
    dev, d, N = _device(images, device), int(size_divisor), len(images)
    flips = [False] * N if flips is None else [bool(f) for f in flips]
    photometric = [None] * N if photometric is None else list(photometric)
    assert len(flips) == N == len(photometric), 'prepare_batch: one flip and one photometric entry per image'
    shapes = [tuple(int(s) for s in im.shape[:2]) for im in images]
    Hb, Wb = max((_round_up(h, d) for h, _ in shapes), default=d), max((_round_up(w, d) for _, w in shapes), default=d)
    img = torch.zeros(N, 3, Hb, Wb, dtype=torch.float32, device=dev)
    coord = torch.zeros(N, 2, Hb, Wb, dtype=torch.float32, device=dev)
    if N == 0:
        return img, coord
    mean32 = host_to_device([float(np.float32(m)) for m in mean], torch.float32, dev)
    inv32 = host_to_device([float(np.float32(1.0 / float(s))) for s in std], torch.float32, dev)
    for n, (image, (h, w)) in enumerate(zip(images, shapes)):
        x = _as_hwc(image, dev).to(torch.float32)
        if flips[n]:
            x = x.flip(1)
        b, g, r = x.unbind(-1)
        p = photometric[n]
        if p is not None:
            if (p.saturation_alpha is not None or p.hue_delta is not None) and not p.hsv:
                raise ValueError('prepare_batch: saturation and hue need the HSV round trip')
            b, g, r = photometric_torch(b, g, r, p)
        chain = (b, g, r)
        perm = (0, 1, 2) if p is None or p.permutation is None else p.permutation
        if tuple(perm) not in PERMUTATIONS:
            raise ValueError(f'prepare_batch: {perm!r} is not a permutation of the three channels')
        planes = [chain[perm[2 - c if to_rgb else c]] for c in range(3)]
        img[n, :, :h, :w] = (torch.stack(planes) - mean32[:, None, None]) * inv32[:, None, None]
        c2d = gen_coord_2d(h, w, d, flips[n], device=dev)[0]
        coord[n, :, :c2d.shape[1], :c2d.shape[2]] = c2d
    return img, coord


# ------------------------------------------------------------------------------------------------ the public function
def _device(images, device):
    if device is not None:
        return torch.device(device)
    for im in images:
        if isinstance(im, torch.Tensor):
            return im.device
    return torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')


def fast_path_reason(images, size_divisor=32, device=None):
    """None when ``mr_image_prepare`` covers the call, else what sends it to the literal path, in words."""
    dev, d = _device(images, device), int(size_divisor)
    if dev.type != 'cuda':
        return f'the device is {dev.type}, the launch runs on a CUDA device'
    for n, im in enumerate(images):
        dtype = im.dtype if isinstance(im, torch.Tensor) else np.asarray(im).dtype
        if dtype != (torch.uint8 if isinstance(im, torch.Tensor) else np.dtype(np.uint8)):
            return f'image {n} is {dtype}, the launch reads uint8'
        if len(im.shape) != 3 or im.shape[2] != 3:
            return f'image {n} has the shape {tuple(im.shape)}, the launch reads (h, w, 3)'
    if d < 4 or d % 4:
        return f'size_divisor {d} is not a positive multiple of 4'
    if len(images) > MAX_IMAGES:
        return f'{len(images)} images, the launch takes {MAX_IMAGES}'
    Hb = max((_round_up(im.shape[0], d) for im in images), default=d)
    Wb = max((_round_up(im.shape[1], d) for im in images), default=d)
    if Hb * Wb > MAX_PIXELS:
        return f'a batch shape of {Hb} x {Wb} is beyond 32-bit indexing'
    return None


def _pack(images, dev):
    """The images as one uint8 device buffer and their byte offsets: host arrays through ONE pinned staging buffer and one copy in stream
    order, device tensors by a device concatenation."""
    sizes = [int(im.shape[0]) * int(im.shape[1]) * 3 for im in images]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if all(not isinstance(im, torch.Tensor) or im.device.type == 'cpu' for im in images):
        stage = torch.empty(int(offsets[-1]), dtype=torch.uint8).pin_memory()
        view = stage.numpy()
        for im, o, s in zip(images, offsets, sizes):
            view[o:o + s] = (im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)).reshape(-1)
        return stage.to(dev, non_blocking=True), offsets
    parts = [(im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im)).pin_memory()).to(dev, non_blocking=True)
             .contiguous().reshape(-1) for im in images]
    return torch.cat(parts), offsets


def image_metas(shapes, mean, std, to_rgb, size_divisor, flips, filenames=None):
    """mmdet's ``img_metas`` as ``Collect`` leaves them, one dict per image."""
    d = int(size_divisor)
    metas = []
    for n, (h, w) in enumerate(shapes):
        name = None if filenames is None else filenames[n]
        metas.append(dict(filename=name, ori_filename=name, ori_shape=(h, w, 3), img_shape=(h, w, 3), pad_shape=(_round_up(h, d), _round_up(w, d), 3),
                          scale_factor=np.ones(4, dtype=np.float32), flip=bool(flips[n]), flip_direction='horizontal' if flips[n] else None,
                          img_norm_cfg=dict(mean=np.array(mean, dtype=np.float32), std=np.array(std, dtype=np.float32), to_rgb=bool(to_rgb))))
    return metas


def prepare_batch(images, mean, std, to_rgb=True, size_divisor=32, flips=None, photometric=None, device=None, path=None, filenames=None):
    """images: a list of (h, w, 3) arrays or tensors in B, G, R order (uint8 for the launch); mean, std, to_rgb: ``img_norm_cfg``;
    size_divisor: ``Pad3D``'s; flips: per image, default none; photometric: per image a :class:`PhotoParams` or None, default none;
    path: None (the launch where :func:`fast_path_reason` is None, else the literal path), ``'fast'`` (raise that reason) or ``'literal'``.
    -> ``(img (N, 3, Hb, Wb) fp32, coord_2d (N, 2, Hb, Wb) fp32, img_metas)`` on ``device``."""
    global last_path
    if path not in (None, 'fast', 'literal'):
        raise ValueError(f'prepare_batch: path {path!r}')
    images = list(images)
    N, d, dev = len(images), int(size_divisor), _device(images, device)
    flips = [False] * N if flips is None else [bool(f) for f in flips]
    photometric = [None] * N if photometric is None else list(photometric)
    if len(flips) != N or len(photometric) != N:
        raise ValueError('prepare_batch: one flip and one photometric entry per image')
    reason = fast_path_reason(images, d, dev)
    if path == 'fast' and reason is not None:
        raise RuntimeError(f'prepare_batch: path="fast", but {reason}')
    shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    metas = image_metas(shapes, mean, std, to_rgb, d, flips, filenames)
    if path == 'literal' or reason is not None:
        img, coord = prepare_batch_torch(images, mean, std, to_rgb, d, flips, photometric, dev)
        last_path = 'literal'
        return img, coord, metas
    if N == 0:
        img, coord = image_prepare(torch.empty(0, dtype=torch.uint8, device=dev), np.zeros((0, TABLE_WORDS), np.int32), mean, std, to_rgb, d)
    else:
        src, offsets = _pack(images, dev)
        rows = np.stack([table_row(offsets[n], h, w, 3 * w, flips[n], photometric[n]) for n, (h, w) in enumerate(shapes)])
        img, coord = image_prepare(src, rows, mean, std, to_rgb, d)
    last_path = 'fast'
    return img, coord, metas


def prepare_train_batch(samples, rng, mean, std, to_rgb=True, size_divisor=32, device=None, path=None, **augmentation):
    """samples: a list of dicts holding ``img`` (uint8 (h, w, 3) B, G, R), ``gt_bboxes`` (G, 4), ``gt_labels`` (G,), ``gt_bboxes_3d``
    (G, 7), ``cam_intrinsic`` (3, 3) and optionally ``gt_bboxes_ignore`` (.., 4); rng: a ``numpy.random.RandomState``, from which each
    image's flip and photometric parameters are drawn in turn (:func:`draw_augmentation`, which takes ``augmentation``).  -> the keyword
    dict of ``MonoRUnDetector.forward(return_loss=True, **data)``: ``img``, ``img_metas``, ``gt_bboxes``, ``gt_bboxes_ignore``,
    ``gt_labels``, ``gt_bboxes_3d``, ``coord_2d``, ``cam_intrinsic``.  The 2-D boxes are flipped where the image is; ``gt_bboxes_3d`` and
    ``cam_intrinsic`` pass through untouched, as ``RandomFlip3D`` leaves them (the heads read the flip from ``img_metas``)."""
    samples = list(samples)
    dev = _device([s['img'] for s in samples], device)
    drawn = [draw_augmentation(rng, **augmentation) for _ in samples]
    flips, photo = [f for f, _ in drawn], [p for _, p in drawn]
    img, coord, metas = prepare_batch([s['img'] for s in samples], mean, std, to_rgb, size_divisor, flips, photo, dev, path)

    def tensor(v, dtype, shape):
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        t = t.to(dtype).reshape(shape)
        return t.pin_memory().to(dev, non_blocking=True) if dev.type == 'cuda' and t.device.type == 'cpu' else t.to(dev)

    data = dict(img=img, img_metas=metas, gt_bboxes=[], gt_bboxes_ignore=[], gt_labels=[], gt_bboxes_3d=[], coord_2d=coord)
    for s, m in zip(samples, metas):
        boxes = tensor(s['gt_bboxes'], torch.float32, (-1, 4))
        ignore = tensor(s['gt_bboxes_ignore'] if s.get('gt_bboxes_ignore') is not None else np.zeros((0, 4), np.float32), torch.float32, (-1, 4))
        if m['flip']:
            boxes, ignore = flip_bboxes(boxes, m['img_shape']), flip_bboxes(ignore, m['img_shape'])
        data['gt_bboxes'].append(boxes)
        data['gt_bboxes_ignore'].append(ignore)
        data['gt_labels'].append(tensor(s['gt_labels'], torch.int64, (-1,)))
        data['gt_bboxes_3d'].append(tensor(s['gt_bboxes_3d'], torch.float32, (-1, 7)))
    data['cam_intrinsic'] = torch.stack([tensor(s['cam_intrinsic'], torch.float32, (3, 3)) for s in samples]) if samples else \
        torch.zeros(0, 3, 3, device=dev)
    return data


# ------------------------------------------------------------------------------------------------ the reference's apis/inference.py
def _cfg(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _find_transform(pipeline, names):
    """The first transform of a pipeline (nested ``transforms`` included, as under ``MultiScaleFlipAug``) whose type is one of ``names``."""
    for step in pipeline or ():
        if _cfg(step, 'type') in names:
            return step
        found = _find_transform(_cfg(step, 'transforms'), names)
        if found is not None:
            return found
    return None


def test_pipeline_settings(cfg):
    """``(mean, std, to_rgb, size_divisor)`` of ``cfg.data.test.pipeline``: its ``Normalize`` and its ``Pad3D`` / ``Pad``."""
    pipeline = _cfg(_cfg(_cfg(cfg, 'data'), 'test'), 'pipeline')
    if pipeline is None:
        raise ValueError('inference_detector: model.cfg has no data.test.pipeline')
    norm, pad = _find_transform(pipeline, ('Normalize',)), _find_transform(pipeline, ('Pad3D', 'Pad'))
    if norm is None:
        raise ValueError('inference_detector: the test pipeline has no Normalize')
    divisor = _cfg(pad, 'size_divisor') if pad is not None else None
    if pad is not None and divisor is None:
        raise NotImplementedError('inference_detector: a Pad to a fixed size is not provided, only size_divisor')
    return _cfg(norm, 'mean'), _cfg(norm, 'std'), bool(_cfg(norm, 'to_rgb', True)), int(divisor) if divisor else 4


test_pipeline_settings.__test__ = False            # a public helper, not a test


def init_detector(config, checkpoint=None, device='cuda:0'):
    """The reference's ``init_detector`` (apis/inference.py:16-48) without mmcv: ``config`` is a dict or an object with ``model`` and
    ``test_cfg`` (a config FILE is Python that mmcv executes: load it yourself and pass the result); ``checkpoint`` a LOCAL file of
    ``torch.save`` (its ``state_dict`` entry, or the mapping itself; a URL raises, nothing is fetched).  The model is built through
    :class:`MonoRUnDetector` with ``pretrained=None``, keeps ``config`` as ``model.cfg``, moves to ``device`` and is put in eval mode."""
    from .detector import MonoRUnDetector
    if isinstance(config, (str, bytes, os.PathLike)):
        raise TypeError('init_detector: config is a dict or an object, not a file name: a config file is code for mmcv.Config to run')
    model_cfg = dict(_cfg(config, 'model') or {})
    if not model_cfg:
        raise TypeError('init_detector: config has no model')
    typ = model_cfg.pop('type', 'MonoRUnDetector')
    if typ != 'MonoRUnDetector':
        raise KeyError(f'init_detector: {typ}: the model is a MonoRUnDetector')
    model_cfg['pretrained'] = None
    model_cfg.pop('train_cfg', None)
    test_cfg = model_cfg.pop('test_cfg', None) or _cfg(config, 'test_cfg')
    model = MonoRUnDetector(**model_cfg, test_cfg=test_cfg)
    if checkpoint is not None:
        if not isinstance(checkpoint, (str, bytes, os.PathLike)) or '://' in str(checkpoint):
            raise ValueError(f'init_detector: {checkpoint!r} would have to be fetched; download the checkpoint and pass its local path')
        loaded = torch.load(checkpoint, map_location='cpu')
        state = loaded.get('state_dict', loaded) if isinstance(loaded, dict) else loaded
        state = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state.items()}
        model.load_state_dict(state, strict=False)
        meta = loaded.get('meta') if isinstance(loaded, dict) else None
        if isinstance(meta, dict) and 'CLASSES' in meta:
            model.CLASSES = meta['CLASSES']
    model.cfg = config
    model.to(device)
    model.eval()
    return model


def inference_detector(model, img, calib=None):
    """The reference's ``inference_detector`` (apis/inference.py:78-120) for one image: ``img`` a file name (:func:`load_image`) or a uint8
    (h, w, 3) B, G, R array; ``calib`` the (3, 3) camera matrix, which the 3-D heads need.  The normalisation and ``size_divisor`` come from
    ``model.cfg.data.test.pipeline``; the image is prepared on the model's device (:func:`prepare_batch`) and the result is
    ``model(return_loss=False, rescale=True, ...)``."""
    if isinstance(img, (list, tuple)):
        raise NotImplementedError('inference_detector: one image per call')
    if calib is None:
        raise ValueError('inference_detector: calib (the 3 x 3 camera matrix) is needed for the 3-D result')
    mean, std, to_rgb, divisor = test_pipeline_settings(model.cfg)
    device = next(model.parameters()).device
    name = os.fspath(img) if isinstance(img, (str, os.PathLike)) else None
    image = load_image(name) if name is not None else img
    batch, coord_2d, metas = prepare_batch([image], mean, std, to_rgb, divisor, device=device, filenames=[name])
    cam = torch.as_tensor(np.asarray(calib.detach().cpu() if isinstance(calib, torch.Tensor) else calib, dtype=np.float32).reshape(1, 3, 3))
    cam = cam.pin_memory().to(device, non_blocking=True) if device.type == 'cuda' else cam.to(device)
    with torch.no_grad():
        return model(return_loss=False, rescale=True, img=[batch], img_metas=[metas], coord_2d=[coord_2d], cam_intrinsic=[cam])
