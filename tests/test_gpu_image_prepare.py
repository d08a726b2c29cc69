"""The image preparation on the GPU: ``mr_image_prepare`` bitwise against the per-pixel numpy restatement
(tests/image_prepare_ref.py) and against the literal path on the device, launched under torch's synchronisation debug mode — every size at
which the kernel takes another path, a batch of unequal images, strided sources at odd offsets, every photometric flavour —, then
``inference_detector`` against the parts by hand and ``prepare_train_batch`` through ``train_step`` on the reduced-width detector."""
import copy

import numpy as np
import pytest
import torch

from tests import image_prepare_ref as ref
from tests import roi_head_ref as rr
from tests import roi_train_ref as tr
from monorun_amd import image_pipeline as ip

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
MASK_SEED = 1234


class no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode('default')


def same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name', ref.CASES)
def test_launch_equals_the_restatement_and_the_literal_path_bitwise_without_a_synchronisation(name):
    args = ref.call_args(name)
    want_img, want_coord, reached = ref.expected(name)
    assert ip.fast_path_reason(args['images'], device=DEV) is None
    ip.prepare_batch(**args, device=DEV, path='fast')                             # warm-up: the library, the pinned allocator
    with no_sync():
        img, coord, metas = ip.prepare_batch(**args, device=DEV, path='fast')
        assert ip.last_path == 'fast'
        again_img, again_coord, _ = ip.prepare_batch(**args, device=DEV)          # a repeated call into fresh buffers
        assert ip.last_path == 'fast'
    lit_img, lit_coord, _ = ip.prepare_batch(**args, device=DEV, path='literal')
    assert ip.last_path == 'literal' and lit_img.device == img.device == DEV and len(metas) == len(args['images'])
    assert img.data_ptr() != again_img.data_ptr() or img.numel() == 0
    assert same_bits(img, want_img) and same_bits(coord, want_coord), 'against the restatement'
    assert same_bits(img, lit_img) and same_bits(coord, lit_coord), 'against the literal path'
    assert same_bits(img, again_img) and same_bits(coord, again_coord), 'a repeated call'
    if name == 'batch3':                                                          # all three regions occur in the first image
        h, w = args['images'][0].shape[:2]
        inside, padded, beyond = want_coord[0, :, :h, :w], want_coord[0, :, h:64, :64], want_coord[0, :, 64:, :]
        assert inside.size and padded.size and beyond.size and (h, w) == (37, 50) and img.shape == (3, 3, 96, 64)
        assert float(np.abs(beyond).sum()) == 0 and padded[1].min() == h - 1 and float(np.abs(want_img[0, :, h:, :]).sum()) == 0
        assert float(coord[0, 0, h - 1, 63]) == w - 1 and float(coord[1, 0, 0, 63]) == 0        # the flipped image's last column holds 0
    if name == 'flavours-rgb':
        assert {'H:r', 'H:g', 'H:b', 'H<0', 'S>1', 'hue>360', 'hue<0', 'S=0', 'd=0', 'black'} | {f'sector:{s}' for s in range(6)} <= reached, sorted(reached)
    if name == 'empty':
        assert img.shape == (0, 3, 32, 32) and coord.shape == (0, 2, 32, 32)
    if name == 'many':
        assert img.shape == (40, 3, 32, 32)


def test_strided_sources_at_odd_offsets():
    """the launch on a buffer it did not pack: row strides above 3 w, odd byte offsets, a batch shape larger than any image needs"""
    c = ref.case('batch3')
    buf, layout, views = ref.in_buffer(c['images'])
    assert all(o % 2 == 1 for o, _ in layout) and any(s > 3 * im.shape[1] for (_, s), im in zip(layout, c['images']))
    assert all(np.array_equal(v, im) for v, im in zip(views, c['images']))
    rows = np.stack([ip.table_row(o, im.shape[0], im.shape[1], s, flip, ref.params(p))
                     for (o, s), im, flip, p in zip(layout, c['images'], c['flips'], c['photos'])])
    src = torch.from_numpy(buf).to(DEV)
    with no_sync():
        img, coord = ip.image_prepare(src, rows, ref.MEAN, ref.STD, True, 32)
        wide_img, wide_coord = ip.image_prepare(src, rows, ref.MEAN, ref.STD, True, 32, batch_shape=(128, 96))
    want_img, want_coord, _ = ref.expected('batch3')
    assert same_bits(img, want_img) and same_bits(coord, want_coord)
    assert wide_img.shape == (3, 3, 128, 96) and same_bits(wide_img[:, :, :96, :64], want_img) and same_bits(wide_coord[:, :, :96, :64], want_coord)
    rest = torch.ones(128, 96, dtype=torch.bool, device=DEV)
    rest[:96, :64] = False
    assert float(wide_img[:, :, rest].abs().sum()) == 0 and float(wide_coord[:, :, rest].abs().sum()) == 0
    with pytest.raises(ValueError, match='leaves the buffer'):                   # the wrapper validates before it launches
        ip.image_prepare(src[:-200], rows, ref.MEAN, ref.STD)


def test_what_the_launch_does_not_cover_runs_the_literal_path():
    im = ref.image(33, 65, 6)
    img, coord, _ = ip.prepare_batch([im.astype(np.float32)], ref.MEAN, ref.STD, device=DEV)
    assert ip.last_path == 'literal' and img.device == DEV
    fast = ip.prepare_batch([im], ref.MEAN, ref.STD, device=DEV)
    assert ip.last_path == 'fast' and same_bits(img, fast[0]) and same_bits(coord, fast[1])
    with pytest.raises(RuntimeError, match='uint8'):
        ip.prepare_batch([im.astype(np.float32)], ref.MEAN, ref.STD, device=DEV, path='fast')
    on_device = ip.prepare_batch([torch.from_numpy(im).to(DEV)], ref.MEAN, ref.STD)        # a device tensor: its device, the launch
    assert ip.last_path == 'fast' and same_bits(on_device[0], fast[0])


# ------------------------------------------------------------------------------------------------ the detector
def same_results(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for key in a:
        assert len(a[key]) == len(b[key]) == rr.NUM_CLASSES, key
        for c, (p, q) in enumerate(zip(a[key], b[key])):
            assert same_bits(p, q), (key, c, np.shape(p), np.shape(q))


def test_inference_detector_equals_the_parts_by_hand():
    torch.manual_seed(0)
    model = ip.init_detector(ref.reduced_config(), device=DEV)
    rr.seed_heads(model.roi_head, 0)
    array = ref.image(rr.IMG_H, rr.IMG_W, 7, planted=False)
    calib = np.array([[360.0, 0.0, 160.0], [0.0, 360.0, 48.0], [0.0, 0.0, 1.0]], np.float32)
    torch.manual_seed(MASK_SEED)
    got = ip.inference_detector(model, array, calib)
    assert ip.last_path == 'fast' and model.roi_head.last_path == 'fast'
    img, coord, metas = ip.prepare_batch([array], ref.MEAN, ref.STD, True, 32, device=DEV)
    assert img.shape == (1, 3, rr.IMG_H, rr.IMG_W) and metas[0]['flip'] is False
    torch.manual_seed(MASK_SEED)
    want = model(return_loss=False, rescale=True, img=[img], img_metas=[metas], coord_2d=[coord], cam_intrinsic=[torch.from_numpy(calib).to(DEV)[None]])
    assert isinstance(got, list) and len(got) == 1
    same_results(got[0], want[0])
    print('detections per class:', [len(b) for b in got[0]['bbox_3d_results']])


def train_detector():
    """tests/roi_train_ref.py's detector without the NOC head's LiDAR loss: the sample dicts carry no dense coordinate maps, as in the
    reference's shipped config (with_coord_3d=False)"""
    from monorun_amd.detector import MonoRUnDetector
    torch.manual_seed(0)
    train_cfg = copy.deepcopy(tr.TRAIN_CFG)
    del train_cfg['rcnn']['iou3d_sampler']
    model = rr.model_cfg()
    model['roi_head'] = tr.roi_head_cfg()
    del model['roi_head']['noc_head']['loss_noc']
    model['rpn_head'].update(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                             loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))
    det = MonoRUnDetector(**model, train_cfg=train_cfg, test_cfg=copy.deepcopy(rr.TEST_CFG))
    tr.seed_heads(det.roi_head, 0)
    return det.train().to(DEV)


def train_samples():
    inputs = tr.batch_inputs('cpu', n_images=3)
    return [dict(img=ref.image(h, w, 30 + n, planted=False), gt_bboxes=inputs['gt_bboxes'][n].numpy(), gt_labels=inputs['gt_labels'][n].numpy(),
                 gt_bboxes_ignore=np.zeros((0, 4), np.float32), gt_bboxes_3d=inputs['gt_bboxes_3d'][n].numpy(), cam_intrinsic=tr.CAM)
            for n, (h, w, _) in enumerate(tr.SHAPES)]


def test_train_batch_goes_through_a_training_step():
    det, samples = train_detector(), train_samples()
    seed = next(s for s in range(50) if len({ip.draw_augmentation(r)[0] for r in [np.random.RandomState(s)] for _ in samples}) == 2)
    fast = ip.prepare_train_batch(samples, np.random.RandomState(seed), ref.MEAN, ref.STD, device=DEV)
    assert ip.last_path == 'fast'
    literal = ip.prepare_train_batch(samples, np.random.RandomState(seed), ref.MEAN, ref.STD, device=DEV, path='literal')
    assert ip.last_path == 'literal'
    assert fast['img'].shape == (3, 3, tr.IMG_H, tr.IMG_W) and same_bits(fast['img'], literal['img']) and same_bits(fast['coord_2d'], literal['coord_2d'])
    assert [m['flip'] for m in fast['img_metas']] == [m['flip'] for m in literal['img_metas']] and len({m['flip'] for m in fast['img_metas']}) == 2
    for k in ('gt_bboxes', 'gt_labels', 'gt_bboxes_3d'):
        assert all(same_bits(a, b) for a, b in zip(fast[k], literal[k])), k
    outs, dets = [], []
    for data in (fast, literal):
        dets.append(copy.deepcopy(det))                                           # a training step leaves state behind in the heads: a copy each
        torch.manual_seed(5)
        gen = lambda s: torch.Generator(device=DEV).manual_seed(s)
        outs.append(dets[-1].train_step(dict(data, rpn_kwargs=dict(generator=gen(1)), generator=gen(2))))
    out = outs[0]
    assert out['num_samples'] == 3 and torch.isfinite(out['loss']) and all(np.isfinite(v) for v in out['log_vars'].values())
    upstream = ('loss_rpn_cls', 'loss_rpn_bbox', 'loss_cls', 'acc', 'loss_bbox', 'loss_dim')
    assert set(upstream) | {'loss'} <= set(out['log_vars'])
    print(outs[0]['log_vars'], outs[1]['log_vars'], sep='\n')
    for k in upstream:                                                            # equal inputs, equal losses upstream of the NOC decode
        assert outs[0]['log_vars'][k] == outs[1]['log_vars'][k], k
    out['loss'].backward()
    grads = {n: p.grad for n, p in dets[0].named_parameters() if p.requires_grad and p.grad is not None}
    assert grads and all(torch.isfinite(g).all() for g in grads.values())
    for part in ('backbone.layer2.', 'neck.', 'rpn_head.', 'roi_head.bbox_head.', 'roi_head.global_head.'):      # the image reaches every loss
        assert any(n.startswith(part) and float(g.abs().sum()) > 0 for n, g in grads.items()), part
