"""The image preparation without a GPU: the literal path against the per-pixel numpy restatement (tests/image_prepare_ref.py)
bit for bit, ``coord_2d`` against ``gen_coord_2d`` and fixture G9, ``draw_augmentation`` against mmdet's statements, the boxes, the metas,
the loader's row, the host checks of the entry point and of its Python wrapper, and ``init_detector``."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import image_prepare_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G9 = np.load(os.path.join(ROOT, 'tests', 'golden', 'g9_coord2d.npz'))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the literal path
@pytest.mark.parametrize('name', ref.CASES)
def test_literal_path_equals_the_restatement_bitwise(name):
    from monorun_amd import image_pipeline as ip
    want_img, want_coord, _ = ref.expected(name)
    img, coord, metas = ip.prepare_batch(**ref.call_args(name), device='cpu')
    assert ip.last_path == 'literal' and len(metas) == len(ref.case(name)['images'])
    assert img.dtype == coord.dtype == torch.float32 and img.shape == want_img.shape and coord.shape == want_coord.shape
    assert np.array_equal(bits(img.numpy()), bits(want_img)), 'img'
    assert np.array_equal(bits(coord.numpy()), bits(want_coord)), 'coord_2d'


def test_the_cases_reach_every_branch_of_the_conversions():
    reached = set()
    for name in ('flavours-rgb', 'batch3', 'size-37x50'):
        reached |= ref.expected(name)[2]
    want = {'H:r', 'H:g', 'H:b', 'H<0', 'S>1', 'hue>360', 'hue<0', 'S=0', 'd=0', 'black'} | {f'sector:{s}' for s in range(6)}
    assert want <= reached, sorted(want - reached)
    # the planted pixels alone reach the three H branches and the six sectors through the bare round trip
    alone = set()
    for px in ref.PLANTED:
        ref.photometric_pixel(*(np.float32(v) for v in px), dict(), alone)
    assert {'H:r', 'H:g', 'H:b', 'S=0', 'd=0', 'black'} | {f'sector:{s}' for s in range(6)} <= alone, sorted(alone)


def test_the_round_trip_is_not_the_identity_and_no_photometric_step_skips_it():
    from monorun_amd import image_pipeline as ip
    im = ref.image(12, 20, 9)
    kw = dict(mean=(0, 0, 0), std=(1, 1, 1), to_rgb=False, device='cpu')
    plain = ip.prepare_batch([im], **kw)[0]
    assert np.array_equal(plain[0, :, :12, :20].numpy(), im.transpose(2, 0, 1).astype(np.float32))         # exactly the bytes
    assert torch.equal(ip.prepare_batch([im], photometric=[ip.PhotoParams(hsv=False)], **kw)[0], plain)
    assert not torch.equal(ip.prepare_batch([im], photometric=[ip.PhotoParams()], **kw)[0], plain)
    with pytest.raises(ValueError, match='HSV'):
        ip.prepare_batch([im], photometric=[ip.PhotoParams(hue_delta=3.0, hsv=False)], **kw)


# ------------------------------------------------------------------------------------------------ coord_2d
def test_coord_2d_is_gen_coord_2d_inside_the_padded_shape_and_zero_beyond():
    from monorun_amd import image_pipeline as ip
    from monorun_amd.pose_head import gen_coord_2d
    c = ref.case('batch3')
    _, coord, metas = ip.prepare_batch(**ref.call_args('batch3'), device='cpu')
    assert coord.shape == (3, 2, 96, 64)
    for n, (im, flip) in enumerate(zip(c['images'], c['flips'])):
        h, w = im.shape[:2]
        own = gen_coord_2d(h, w, 32, flip)[0]
        hp, wp = own.shape[1:]
        assert metas[n]['pad_shape'] == (hp, wp, 3)
        assert torch.equal(coord[n, :, :hp, :wp], own)
        beyond = torch.ones(96, 64, dtype=torch.bool)
        beyond[:hp, :wp] = False
        assert float(coord[n][:, beyond].abs().sum()) == 0
    # the three regions of image 0 are there
    h, w = c['images'][0].shape[:2]
    assert h < 64 < 96 and w < 64


def test_coord_2d_equals_the_golden_fixture():
    from monorun_amd import image_pipeline as ip
    seen = 0
    for n, (h, w, flip) in enumerate(G9['cases']):
        if f'map_{n}' not in G9:
            continue
        _, coord, _ = ip.prepare_batch([np.zeros((int(h), int(w), 3), np.uint8)], ref.MEAN, ref.STD, flips=[bool(flip)], device='cpu')
        assert np.array_equal(coord[0].numpy(), G9[f'map_{n}']), (h, w, flip)
        seen += 1
    assert seen >= 4


# ------------------------------------------------------------------------------------------------ the augmentation's draw
def test_draw_augmentation_consumes_the_stream_in_mmdets_order():
    from monorun_amd import image_pipeline as ip
    took = set()
    for seed in range(200):
        a, b = np.random.RandomState(seed), np.random.RandomState(seed)
        flip, p = ip.draw_augmentation(a)
        want_flip, want, branches = ref.mmdet_draw(b)
        took |= branches
        assert flip is want_flip and p.hsv
        for k in ('brightness_delta', 'contrast_alpha', 'saturation_alpha', 'hue_delta', 'permutation'):
            assert getattr(p, k) == want.get(k), (seed, k)
        assert p.contrast_mode == want['contrast_mode']
        assert a.randint(1 << 30) == b.randint(1 << 30), f'seed {seed}: the streams are at different places'
    assert took == ref.ALL_DRAW_BRANCHES, sorted(ref.ALL_DRAW_BRANCHES - took)
    # the ranges are arguments
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    flip, p = ip.draw_augmentation(a, flip_ratio=0.0, brightness_delta=8, contrast_range=(0.9, 1.1), saturation_range=(0.8, 0.9), hue_delta=4)
    _, want, _ = ref.mmdet_draw(b, 0.0, 8, 0.9, 1.1, 0.8, 0.9, 4)
    assert flip is False and all(getattr(p, k) == want.get(k) for k in ('brightness_delta', 'contrast_alpha', 'saturation_alpha', 'hue_delta'))


# ------------------------------------------------------------------------------------------------ boxes, metas, the train batch
def test_flip_bboxes_is_mmdets():
    from monorun_amd.image_pipeline import flip_bboxes
    boxes = np.array([[10, 5, 30, 25], [0, 0, 50, 37]], np.float32)
    want = np.array([[20, 5, 40, 25], [0, 0, 50, 37]], np.float32)
    assert np.array_equal(flip_bboxes(boxes, (37, 50, 3)), want) and boxes[0, 0] == 10
    t = torch.from_numpy(boxes)
    assert torch.equal(flip_bboxes(t, (37, 50, 3)), torch.from_numpy(want)) and t[0, 0] == 10
    assert np.array_equal(flip_bboxes(flip_bboxes(boxes, (37, 50)), (37, 50)), boxes)
    assert flip_bboxes(np.zeros((0, 4), np.float32), (3, 3)).shape == (0, 4)


def test_img_metas_carry_mmdets_keys():
    from monorun_amd import image_pipeline as ip
    _, _, metas = ip.prepare_batch([ref.image(37, 50), ref.image(5, 3)], ref.MEAN, ref.STD, flips=[True, False], device='cpu', filenames=['a.png', None])
    keys = {'filename', 'ori_filename', 'ori_shape', 'img_shape', 'pad_shape', 'scale_factor', 'flip', 'flip_direction', 'img_norm_cfg'}
    assert all(set(m) == keys for m in metas)
    m = metas[0]
    assert m['filename'] == m['ori_filename'] == 'a.png' and m['ori_shape'] == m['img_shape'] == (37, 50, 3) and m['pad_shape'] == (64, 64, 3)
    assert m['flip'] is True and m['flip_direction'] == 'horizontal' and metas[1]['flip'] is False and metas[1]['flip_direction'] is None
    assert m['scale_factor'].dtype == np.float32 and m['scale_factor'].tolist() == [1, 1, 1, 1] and metas[1]['pad_shape'] == (32, 32, 3)
    assert m['img_norm_cfg']['to_rgb'] is True and np.allclose(m['img_norm_cfg']['mean'], ref.MEAN) and np.allclose(m['img_norm_cfg']['std'], ref.STD)


def train_samples():
    cam = np.array([[360.0, 0.0, 160.0], [0.0, 360.0, 48.0], [0.0, 0.0, 1.0]], np.float32)
    out = []
    for n, (h, w) in enumerate(((37, 50), (70, 33), (32, 64), (33, 65))):
        boxes = np.array([[2, 3, 20, 30], [5, 1, w - 1, h - 2]], np.float32)[:1 + n % 2]
        out.append(dict(img=ref.image(h, w, 20 + n), gt_bboxes=boxes, gt_labels=np.arange(len(boxes)), gt_bboxes_ignore=np.array([[1, 1, 4, 4]], np.float32),
                        gt_bboxes_3d=np.arange(7 * len(boxes), dtype=np.float32).reshape(-1, 7) + n, cam_intrinsic=cam + n))
    return out


def test_train_batch_flips_the_boxes_only_where_the_image_is():
    from monorun_amd import image_pipeline as ip
    samples = train_samples()
    seed = next(s for s in range(50) if len({ip.draw_augmentation(r)[0] for r in [np.random.RandomState(s)] for _ in samples}) == 2)
    rng = np.random.RandomState(seed)
    drawn = [ip.draw_augmentation(rng) for _ in samples]
    data = ip.prepare_train_batch(copy.deepcopy(samples), np.random.RandomState(seed), ref.MEAN, ref.STD, device='cpu')
    assert set(data) == {'img', 'img_metas', 'gt_bboxes', 'gt_bboxes_ignore', 'gt_labels', 'gt_bboxes_3d', 'coord_2d', 'cam_intrinsic'}
    flips = [m['flip'] for m in data['img_metas']]
    assert flips == [f for f, _ in drawn] and True in flips and False in flips
    want_img, want_coord, _ = ip.prepare_batch([s['img'] for s in samples], ref.MEAN, ref.STD, flips=flips, photometric=[p for _, p in drawn], device='cpu')
    assert torch.equal(data['img'], want_img) and torch.equal(data['coord_2d'], want_coord)
    for s, flip, boxes, ignore, labels, b3 in zip(samples, flips, data['gt_bboxes'], data['gt_bboxes_ignore'], data['gt_labels'], data['gt_bboxes_3d']):
        w = s['img'].shape[1]
        want = s['gt_bboxes'].copy()
        if flip:
            want[:, 0], want[:, 2] = w - s['gt_bboxes'][:, 2], w - s['gt_bboxes'][:, 0]
        assert np.array_equal(boxes.numpy(), want) and boxes.dtype == torch.float32
        assert np.array_equal(ignore.numpy(), ip.flip_bboxes(s['gt_bboxes_ignore'], s['img'].shape) if flip else s['gt_bboxes_ignore'])
        assert labels.dtype == torch.int64 and np.array_equal(labels.numpy(), s['gt_labels'])
        assert np.array_equal(b3.numpy(), s['gt_bboxes_3d'])                                  # untouched, as RandomFlip3D leaves them
    assert np.array_equal(data['cam_intrinsic'].numpy(), np.stack([s['cam_intrinsic'] for s in samples]))


def test_paths_and_their_reasons():
    from monorun_amd import image_pipeline as ip
    im = ref.image(5, 3)
    assert 'cpu' in ip.fast_path_reason([im], device='cpu')
    with pytest.raises(RuntimeError, match='path="fast", but the device is cpu'):
        ip.prepare_batch([im], ref.MEAN, ref.STD, device='cpu', path='fast')
    with pytest.raises(ValueError, match='path'):
        ip.prepare_batch([im], ref.MEAN, ref.STD, device='cpu', path='quick')
    assert 'uint8' in ip.fast_path_reason([im.astype(np.float32)], device='cuda:0')
    assert '(h, w, 3)' in ip.fast_path_reason([np.zeros((4, 4, 1), np.uint8)], device='cuda:0')
    assert 'multiple of 4' in ip.fast_path_reason([im], size_divisor=6, device='cuda:0')
    assert ip.fast_path_reason([im, torch.from_numpy(im)], device='cuda:0') is None
    # the literal path takes what the launch does not: float images, another divisor
    img, coord, metas = ip.prepare_batch([im.astype(np.float32)], ref.MEAN, ref.STD, size_divisor=6, device='cpu')
    assert img.shape == (1, 3, 6, 6) and metas[0]['pad_shape'] == (6, 6, 3)
    assert np.array_equal(bits(img.numpy()), bits(ref.prepare([im], divisor=6)[0]))
    with pytest.raises(ValueError, match='one flip'):
        ip.prepare_batch([im], ref.MEAN, ref.STD, flips=[True, False], device='cpu')


def test_load_image_reads_bgr_uint8(tmp_path):
    from PIL import Image
    from monorun_amd.image_pipeline import load_image
    bgr = ref.image(7, 9, 3)
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(tmp_path / 'x.png')
    got = load_image(str(tmp_path / 'x.png'))
    assert got.dtype == np.uint8 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, bgr)
    Image.fromarray(bgr[:, :, 0]).save(tmp_path / 'grey.png')                                  # a grey file reads as three equal channels
    grey = load_image(tmp_path / 'grey.png')
    assert grey.shape == (7, 9, 3) and np.array_equal(grey[:, :, 0], bgr[:, :, 0]) and np.array_equal(grey[:, :, 0], grey[:, :, 2])


# ------------------------------------------------------------------------------------------------ the reference's apis
def test_init_detector_builds_from_a_config_and_a_local_checkpoint(tmp_path):
    import types
    from monorun_amd import MonoRUnDetector, image_pipeline as ip
    cfg = ref.reduced_config()
    torch.manual_seed(0)
    model = ip.init_detector(cfg, device='cpu')
    assert isinstance(model, MonoRUnDetector) and model.cfg is cfg and not model.training and model.test_cfg == cfg['test_cfg']
    assert cfg['model']['pretrained'] == 'torchvision://resnet18', 'the config is not edited'
    assert ip.test_pipeline_settings(model.cfg) == (list(ref.MEAN), list(ref.STD), True, 32)
    torch.save(dict(state_dict={'module.' + k: v + 1 if v.dtype.is_floating_point else v for k, v in model.state_dict().items()},
                    meta=dict(CLASSES=('Car',))), tmp_path / 'c.pth')
    as_object = types.SimpleNamespace(model=cfg['model'], test_cfg=cfg['test_cfg'], data=cfg['data'])
    loaded = ip.init_detector(as_object, str(tmp_path / 'c.pth'), device='cpu')
    assert loaded.CLASSES == ('Car',) and loaded.cfg is as_object
    for (k, a), b in zip(model.state_dict().items(), loaded.state_dict().values()):
        assert torch.equal(a + 1 if a.dtype.is_floating_point else a, b), k
    with pytest.raises(ValueError, match='fetched'):
        ip.init_detector(cfg, 'https://example.invalid/c.pth', device='cpu')
    with pytest.raises(TypeError, match='file name'):
        ip.init_detector('configs/kitti_car.py')
    with pytest.raises(ValueError, match='calib'):
        ip.inference_detector(model, ref.image(5, 3))
    with pytest.raises(ValueError, match='Normalize'):
        ip.test_pipeline_settings(dict(data=dict(test=dict(pipeline=[dict(type='Pad3D', size_divisor=32)]))))


def test_exports():
    import monorun_amd
    for name in ('prepare_batch', 'prepare_batch_torch', 'prepare_train_batch', 'PhotoParams', 'draw_augmentation', 'flip_bboxes', 'load_image',
                 'init_detector', 'inference_detector'):
        assert getattr(monorun_amd, name) is getattr(monorun_amd.image_pipeline, name), name


# ------------------------------------------------------------------------------------------------ the loader's row
_PINNED = ('mr_image_prepare',)
_SCALAR = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64}


def _declared_prototypes(path):
    """[(return type, name, [arguments])] of a header, by a regex of this file's own (not `_lib.header_prototypes`)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(path).read(), flags=re.S)
    found = re.findall(r'^((?:const\s+)?\w+[\s\*]+)(\w+)\s*\(([^)]*)\)\s*;', src, flags=re.M)
    return [(' '.join(ret.split()), name, [] if args.strip() in ('', 'void') else [' '.join(a.split()) for a in args.split(',')])
            for ret, name, args in found]


def header_constants():
    text = open(os.path.join(ROOT, 'include', 'monorun_image.h')).read()
    return {k: int(v, 0) for k, v in re.findall(r'^#define (MR_IMAGE_\w+) (\w+)', text, flags=re.M)}


def test_loader_binds_the_image_header(monkeypatch):
    """the row of `_lib.LATER_HEADERS` this subsystem owns (nothing is asserted about the table's other rows): the pinned names are what the
    header declares, in order, and no other header's; the library exports each; restype, argtypes and arg_names are the declared ones; the
    header alone makes the library stale; the module's constants are the header's"""
    from monorun_amd import _lib, image_pipeline as ip
    key = 'image'
    assert key in _lib.LATER_HEADERS and key in _lib.all_header_keys() and key not in _lib.header_keys()
    assert not set(_PINNED) & set(_lib.exported_symbols())
    lib, raw = _lib.load(), ctypes.CDLL(_lib.SO)
    assert _lib.exported_symbols(key) == _lib.LATER_HEADERS[key][1] == _PINNED
    assert _lib.header_path(key) == os.path.join(ROOT, 'include', 'monorun_image.h')
    assert [n for n, _, _ in _lib.header_prototypes(_lib.header_path(key))] == list(_PINNED)
    declared = _declared_prototypes(_lib.header_path(key))
    assert [name for _, name, _ in declared] == list(_PINNED)
    for other in _lib.all_header_keys():
        if other != key:
            assert not set(_PINNED) & set(_lib.exported_symbols(other)), other
            assert not set(_PINNED) & {n for _, n, _ in _declared_prototypes(_lib.header_path(other))}, other
    for ret, name, args in declared:
        assert hasattr(raw, name), f'{name} declared but not exported'
        f = getattr(lib, name)
        names = [re.search(r'\w+$', a).group() for a in args]
        types = [a.replace('const ', '')[:-len(n)].strip() for a, n in zip(args, names)]
        assert len(set(names)) == len(names) and names[-1] == 'stream'
        assert list(_lib.arg_names(name)) == names[:-1], name
        assert f.restype is _SCALAR[ret], name
        assert list(f.argtypes) == [ctypes.c_void_p if '*' in t else _SCALAR[t] for t in types], name
    assert _lib.table_args('mr_image_prepare') == ()
    v = header_constants()
    assert v['MR_IMAGE_MAX_IMAGES'] == ip.MAX_IMAGES and v['MR_IMAGE_MAX_PIXELS'] == ip.MAX_PIXELS and v['MR_IMAGE_TABLE_WORDS'] == ip.TABLE_WORDS
    assert (v['MR_IMAGE_SW_BRIGHTNESS'], v['MR_IMAGE_SW_CONTRAST'], v['MR_IMAGE_SW_CONTRAST_FIRST'], v['MR_IMAGE_SW_SATURATION'], v['MR_IMAGE_SW_HUE'],
            v['MR_IMAGE_SW_HSV']) == (ip.SW_BRIGHTNESS, ip.SW_CONTRAST, ip.SW_CONTRAST_FIRST, ip.SW_SATURATION, ip.SW_HUE, ip.SW_HSV)
    row = ip.table_row(2 ** 33 + 5, 7, 9, 30, True, ip.PhotoParams(brightness_delta=1.5, contrast_mode=1, contrast_alpha=2.0, permutation=(2, 0, 1)))
    assert row.dtype == np.int32 and row.shape == (v['MR_IMAGE_TABLE_WORDS'],)
    assert (row[v['MR_IMAGE_OFFSET_LO']], row[v['MR_IMAGE_OFFSET_HI']]) == (5, 2) and row[v['MR_IMAGE_H']] == 7 and row[v['MR_IMAGE_W']] == 9
    assert row[v['MR_IMAGE_STRIDE']] == 30 and row[v['MR_IMAGE_FLIP']] == 1 and row[v['MR_IMAGE_PERMUTATION']] == 2 | 0 << 2 | 1 << 4
    assert row[v['MR_IMAGE_SWITCHES']] == ip.SW_BRIGHTNESS | ip.SW_CONTRAST | ip.SW_CONTRAST_FIRST | ip.SW_HSV
    assert row[v['MR_IMAGE_BRIGHTNESS_DELTA']] == np.float32(1.5).view(np.int32) and row[v['MR_IMAGE_CONTRAST_ALPHA']] == np.float32(2.0).view(np.int32)
    assert ip.table_row(0, 1, 1, 3)[v['MR_IMAGE_PERMUTATION']] == v['MR_IMAGE_PERMUTATION_IDENTITY'] and not row[12:].any()
    assert not _lib._stale()
    so_time, real = os.path.getmtime(_lib.SO), os.path.getmtime
    monkeypatch.setattr(os.path, 'getmtime', lambda f: so_time + 10 if f == _lib.header_path(key) else real(f))
    assert _lib._stale()


# ------------------------------------------------------------------------------------------------ the host checks
BAD, UNSUPPORTED = -1, -2


def _checks():
    """(name, overrides of the call, overrides of image 0's row, the code the entry point returns, the wrapper's exception and words)"""
    from monorun_amd import image_pipeline as ip
    return [
        ('zero height', {}, dict(h=0), BAD, ValueError, 'size'),
        ('negative width', {}, dict(w=-3), BAD, ValueError, 'size'),
        ('stride below 3 w', {}, dict(stride=3 * 50 - 1), BAD, ValueError, 'stride'),
        ('offset past the buffer', {}, dict(offset=10 ** 6), BAD, ValueError, 'leaves the buffer'),
        ('negative offset', {}, dict(offset=-1), BAD, ValueError, 'leaves the buffer'),
        ('last row past the buffer', dict(src_bytes=37 * 150 - 1), {}, BAD, ValueError, 'leaves the buffer'),
        ('batch height below the padded shape', dict(batch_h=32), {}, BAD, ValueError, 'beyond the batch shape'),
        ('batch width below the padded shape', dict(batch_w=32), {}, BAD, ValueError, 'beyond the batch shape'),
        ('batch height no multiple', dict(batch_h=80), {}, BAD, ValueError, 'multiple of size_divisor'),
        ('batch width no multiple', dict(batch_w=100), {}, BAD, ValueError, 'multiple of size_divisor'),
        ('divisor no multiple of 4', dict(size_divisor=6, batch_h=66, batch_w=66), {}, BAD, ValueError, 'multiple of 4'),
        ('divisor zero', dict(size_divisor=0), {}, BAD, ValueError, 'multiple of 4'),
        ('a repeated channel', {}, dict(perm=(0, 0, 1)), BAD, ValueError, 'one of the six'),
        ('a fourth channel', {}, dict(perm=(0, 1, 3)), BAD, ValueError, 'one of the six'),
        ('hue without the round trip', {}, dict(photo=ip.PhotoParams(hue_delta=1.0, hsv=False)), BAD, ValueError, 'HSV'),
        ('a parameter that is not finite', {}, dict(photo=ip.PhotoParams(brightness_delta=float('inf'))), BAD, ValueError, 'not finite'),
        ('std zero', dict(std=(1.0, 0.0, 1.0)), {}, BAD, ValueError, 'std'),
        ('mean not finite', dict(mean=(float('nan'), 0.0, 0.0)), {}, BAD, ValueError, 'mean'),
        ('too large a batch shape', dict(batch_h=1 << 16, batch_w=1 << 16), {}, UNSUPPORTED, NotImplementedError, '32-bit'),
    ]


def _call(over, row_over):
    from monorun_amd import image_pipeline as ip
    r = dict(offset=0, h=37, w=50, stride=150, flip=False, photo=None, perm=None)
    r.update(row_over)
    rows = np.stack([ip.table_row(r['offset'], r['h'], r['w'], r['stride'], r['flip'], r['photo']), ip.table_row(37 * 150, 5, 3, 9)])
    if r['perm'] is not None:
        rows[0, 7] = r['perm'][0] | r['perm'][1] << 2 | r['perm'][2] << 4
    a = dict(src_bytes=37 * 150 + 45, size_divisor=32, batch_h=64, batch_w=64, mean=ref.MEAN, std=ref.STD, n_images=2)
    a.update(over)
    return rows, a


@pytest.mark.parametrize('check', range(19))
def test_host_checks_reject_without_a_launch(check):
    """the entry point returns its code before any HIP call (no device is present, and the data pointers are never dereferenced), and the
    Python wrapper's validation raises for the same table"""
    from monorun_amd import _lib, image_pipeline as ip
    assert len(_checks()) == 19
    name, over, row_over, code, exc, words = _checks()[check]
    rows, a = _call(over, row_over)
    d3 = ctypes.c_double * 3
    lib, one = _lib.load(), ctypes.c_void_p(256)
    args = dict(a, src=one, table=rows.ctypes.data, table_device=one, mean=d3(*a['mean']), std=d3(*a['std']), to_rgb=1, img=one, coord_2d=one)
    assert lib.mr_image_prepare(*_lib.pack('mr_image_prepare', args), None) == code, name
    with pytest.raises(exc, match=words):
        ip.check_table(rows, a['src_bytes'], a['size_divisor'], (a['batch_h'], a['batch_w']), a['mean'], a['std'])


def test_host_checks_accept_the_table_they_are_varied_from_and_more():
    from monorun_amd import _lib, image_pipeline as ip
    rows, a = _call({}, {})
    ip.check_table(rows, a['src_bytes'], a['size_divisor'], (a['batch_h'], a['batch_w']), a['mean'], a['std'])
    d3 = ctypes.c_double * 3
    lib, one = _lib.load(), ctypes.c_void_p(256)
    args = dict(a, src=one, table=rows.ctypes.data, table_device=one, mean=d3(*a['mean']), std=d3(*a['std']), to_rgb=1, img=one, coord_2d=one)
    call = lambda **over: lib.mr_image_prepare(*_lib.pack('mr_image_prepare', dict(args, **over)), None)
    assert call(n_images=0) == 0 and call(n_images=0, src=None, table=None, table_device=None, img=None, coord_2d=None) == 0       # nothing is launched
    assert call(n_images=-1) == BAD and call(n_images=65536) == UNSUPPORTED
    assert call(src=None) == BAD and call(table=None) == BAD and call(table_device=None) == BAD and call(img=None) == BAD and call(coord_2d=None) == BAD
    assert call(img=ctypes.c_void_p(260)) == BAD and call(coord_2d=ctypes.c_void_p(264)) == BAD and call(mean=None) == BAD and call(std=None) == BAD
    assert call(src_bytes=-1) == BAD
    with pytest.raises(NotImplementedError, match='images'):
        ip.check_table(np.zeros((65536, 16), np.int32), 0, 32, (32, 32))
    with pytest.raises(TypeError, match='CUDA'):
        ip.image_prepare(torch.zeros(10, dtype=torch.uint8), rows, ref.MEAN, ref.STD)
