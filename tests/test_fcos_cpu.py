"""CPU tests (-m "not gpu") of the FCOS baseline: the recipe builds and equals the reference's, its parameters are the
reference's, the refused settings raise with their names, the torch host mirror of FCOSHead.get_bboxes / get_targets / loss
reproduces what the reference computed (tests/golden/g28_fcos.npz, made by tests/golden/make_golden_fcos.py), and the
float64 restatement (tests/fcos_ref64.py) is pinned to the fixture before the GPU tests lean on it."""
import json
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, build_head
from brcnn.config import ConfigDict
from oracle import orc
from tests import fcos_inputs as fi
from tests import fcos_ref64 as R

G = os.path.join(os.path.dirname(__file__), 'golden', 'g28_fcos.npz')
REF_CONFIG = '/root/reference/configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_coco.py'
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(fi.CONFIG).model)


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(fi.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, fi.SCALES):
            s.scale.fill_(v)
    return head


def test_config_builds_the_baseline(model):
    from brcnn.dense_heads import FCOSHead
    from brcnn.detectors import FCOS, SingleStageDetector
    from brcnn.necks import FPN
    assert type(model) is FCOS and isinstance(model, SingleStageDetector)
    assert type(model.bbox_head) is FCOSHead and type(model.neck) is FPN
    h = model.bbox_head
    assert h.cls_out_channels == 4 and h.strides == fi.STRIDES and h.stacked_convs == 4
    assert h.regress_ranges == ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8))
    assert not (h.center_sampling or h.norm_on_bbox or h.centerness_on_reg) and h.center_sample_radius == 1.5
    assert (h.loss_cls.gamma, h.loss_cls.alpha) == (2.0, 0.25) and type(h.loss_bbox).__name__ == 'IoULoss'
    assert h.loss_bbox.mode == 'log' and h.loss_centerness.use_sigmoid
    assert h.test_cfg.nms_pre == 1000 and h.test_cfg.max_per_img == 100 and h.test_cfg.score_thr == 0.05
    assert not model.with_rpn and not model.with_roi_head and not h.supports_tta
    h._check_limits(h.test_cfg, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])       # the recipe's sizes (800 x 1344)
    cfg = Config.fromfile(fi.CONFIG)
    assert cfg.optimizer.paramwise_cfg == dict(bias_lr_mult=2., bias_decay_mult=0.) and cfg.lr_config.warmup == 'constant'
    assert cfg.optimizer_config == dict(grad_clip=dict(max_norm=35, norm_type=2)) and cfg.img_norm_cfg.to_rgb is False
    assert 'configs/fcos' in open(os.path.join(fi.ROOT, 'tools', 'bench_recipes.py')).read()


@pytest.mark.skipif(not os.path.isfile(REF_CONFIG), reason='reference tree absent')
def test_shipped_config_equals_the_reference_config():
    """the reference recipe loads UNCHANGED through this repo's loader and equals the shipped rewrite key for key"""
    r = Config.fromfile(REF_CONFIG).to_dict()
    assert 'model' in r and r['model']['type'] == 'FCOS'
    assert Config.fromfile(fi.CONFIG).to_dict() == r


def test_parameter_names_and_shapes_are_the_references(model, gold):
    sd = model.state_dict()
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want
    assert list(sd) == [str(k) for k in gold['state_keys']]
    h = build_head(ConfigDict(fi.head_cfg(num_classes=3, in_channels=16, feat_channels=32, stacked_convs=1)))
    assert [k for k in h.state_dict()] == [
        'cls_convs.0.conv.weight', 'cls_convs.0.gn.weight', 'cls_convs.0.gn.bias',
        'reg_convs.0.conv.weight', 'reg_convs.0.gn.weight', 'reg_convs.0.gn.bias',
        'conv_cls.weight', 'conv_cls.bias', 'conv_reg.weight', 'conv_reg.bias', 'conv_centerness.weight',
        'conv_centerness.bias', 'scales.0.scale', 'scales.1.scale', 'scales.2.scale', 'scales.3.scale', 'scales.4.scale']
    assert h.conv_cls.weight.shape == (3, 32, 3, 3) and h.conv_reg.weight.shape == (4, 32, 3, 3)
    assert h.conv_centerness.weight.shape == (1, 32, 3, 3) and h.scales[0].scale.shape == ()
    # Normal(0, 0.01) convs, zero biases but conv_cls's, which starts at the prior 0.01
    assert torch.allclose(h.conv_cls.bias, torch.full((3,), -float(np.log(99.0))))
    assert float(h.conv_reg.bias.detach().abs().max()) == 0 and 0.005 < float(h.cls_convs[0].conv.weight.detach().std()) < 0.02


REFUSED = [
    (dict(norm_cfg=None), 'norm_cfg'),
    (dict(norm_cfg=dict(type='BN', requires_grad=True)), 'norm_cfg'),
    (dict(conv_bias=True), 'conv_bias'),
    (dict(dcn_on_last_conv=True), 'dcn_on_last_conv=True'),
    (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)), 'use_sigmoid=False'),
    (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)), 'loss_cls'),
    (dict(loss_bbox=dict(type='L1Loss', loss_weight=1.0)), 'loss_bbox'),
    (dict(loss_bbox=dict(type='IoULoss', mode='linear', loss_weight=1.0)), 'loss_bbox'),
    (dict(loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)), 'loss_centerness'),
    (dict(loss_centerness=dict(type='MSELoss', loss_weight=1.0)), 'loss_centerness'),
    (dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, reduction='sum')), 'reduction'),
    (dict(loss_bbox=dict(type='GIoULoss', reduction='sum')), 'reduction'),
    (dict(test_cfg=dict(fi.TEST_CFG, nms=dict(type='soft_nms', iou_threshold=0.5))), 'soft'),
    (dict(test_cfg=dict(fi.TEST_CFG, nms=dict(type='nms', iou_threshold=0.5, class_agnostic=True))), 'class_agnostic'),
]


@pytest.mark.parametrize('over,name', REFUSED, ids=[f'{i}-{n}' for i, (_, n) in enumerate(REFUSED)])
def test_refused_settings_raise_with_their_name(over, name):
    with pytest.raises(NotImplementedError, match=name):
        build_head(ConfigDict(fi.head_cfg(**over)))


def test_refused_calls_raise_with_their_name(model):
    head = build()
    cls, raw, ctr = fi.head_outputs(3)
    with pytest.raises(NotImplementedError, match='with_nms=False'):
        head.get_bboxes(cls, fi.decoded(raw, fi.SCALES, False, False), ctr, fi.metas(), with_nms=False)
    with pytest.raises(NotImplementedError, match='gt_bboxes_ignore'):
        head.forward_train_nhwc(None, fi.metas(), None, None, gt_bboxes_ignore=[torch.zeros(0, 4)] * 2)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(fi.TEST_CFG, nms_pre=5000), fi.SIZES)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(fi.TEST_CFG, nms_pre=-1), fi.SIZES)
    imgs = [torch.zeros(1, 3, fi.H, fi.W), torch.zeros(1, 3, fi.H, fi.W)]
    metas = [fi.metas(1), [dict(fi.metas(1)[0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.forward_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        head.aug_test(None, metas)


def test_giou_loss_is_the_references_definition():
    from brcnn.losses import GIoULoss
    from brcnn.registry import LOSSES
    assert LOSSES.get('GIoULoss') is GIoULoss and GIoULoss().eps == 1e-6
    pred = torch.tensor([[0., 0., 2., 2.], [0., 0., 1., 1.], [0., 0., 1., 1.]], requires_grad=True)
    target = torch.tensor([[1., 1., 3., 3.], [2., 2., 3., 3.], [0., 0., 1., 1.]])
    # iou 1/7, hull 9: giou = 1/7 - 2/9; disjoint unit boxes, hull 9: giou = -7/9; identical: 1
    want = torch.tensor([1 - (1 / 7 - 2 / 9), 1 + 7 / 9, 0.0])
    got = GIoULoss(reduction='mean')(pred, target, reduction_override='none')
    assert torch.allclose(got, want, atol=1e-6)
    w = torch.tensor([0.5, 2.0, 1.0])
    assert torch.allclose(GIoULoss(loss_weight=2.0)(pred, target, weight=w, avg_factor=4.0), 2.0 * (want * w).sum() / 4.0)
    assert GIoULoss()(pred, target, weight=torch.zeros(3)).item() == 0.0       # the all-zero-weight shortcut


# ------------------------------------------------------------------------------------------- host mirror vs the fixture
CASES = [(c, name) for c in fi.CLASS_COUNTS for name in ('plain', 'rescale', 'norm')] + [(4, 'empty')]


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_host_mirror_reproduces_the_reference(gold, C, name):
    seed = int(gold[f'seed_bboxes_c{C}'])
    norm = name == 'norm'
    head = build(C, norm_on_bbox=norm)
    cls, raw, ctr = fi.head_outputs(seed, C, norm_on_bbox=norm, empty=(name == 'empty'))
    res = head.get_bboxes(cls, fi.decoded(raw, fi.SCALES, norm, False), ctr, fi.metas(), rescale=(name != 'plain'),
                          batched_nms=orc.batched_nms)
    for b, (det, lab) in enumerate(res):
        want_d, want_l = gold[f'bboxes_c{C}_{name}_det{b}'], gold[f'bboxes_c{C}_{name}_lab{b}']
        assert lab.tolist() == want_l.tolist(), (C, name, b)
        assert det.shape == want_d.shape and np.allclose(det.numpy(), want_d, rtol=0, atol=1e-5), (C, name, b)
    if name == 'empty':
        assert len(res[1][0]) == 0 and len(res[0][0]) > 0


TARGET_CASES = {'plain': dict(), 'center': dict(center_sampling=True, center_sample_radius=fi.RADIUS),
                'norm': dict(norm_on_bbox=True)}


@pytest.mark.parametrize('tag', list(TARGET_CASES))
def test_get_targets_host_mirror_is_exact(gold, tag):
    seed = int(gold['seed_targets'])
    head = build(4, True, **TARGET_CASES[tag])
    gt_bboxes, gt_labels = fi.gts(seed)
    labels, targets = head.get_targets(head.get_points(fi.SIZES, torch.float32, 'cpu'), gt_bboxes, gt_labels)
    for l in range(len(fi.SIZES)):
        assert np.array_equal(labels[l].numpy(), gold[f'targets_{tag}_labels{l}']), (tag, l)
        assert np.array_equal(targets[l].numpy(), gold[f'targets_{tag}_box{l}']), (tag, l)
        assert (labels[l] < 4).any()
    assert not np.array_equal(np.concatenate([gold[f'targets_plain_labels{l}'] for l in range(5)]),
                              np.concatenate([gold[f'targets_center_labels{l}'] for l in range(5)]))


@pytest.mark.parametrize('variant,C', [(v, c) for v in fi.VARIANTS for c in (4, 1)])
def test_loss_host_mirror_reproduces_the_reference(gold, variant, C):
    tag = f'loss_{variant}_c{C}'
    seed = int(gold[f'seed_{tag}'])
    over = fi.VARIANTS[variant]
    norm = bool(over.get('norm_on_bbox', False))
    head = build(C, True, **over)
    cls, raw, ctr = fi.head_outputs(seed, C, norm_on_bbox=norm, grad=True)
    scales = [torch.tensor(v, requires_grad=True) for v in fi.SCALES]
    gt_bboxes, gt_labels = fi.gts(seed, num_classes=C)
    losses = head.loss(cls, fi.decoded(raw, scales, norm, True), ctr, gt_bboxes, gt_labels, fi.metas())
    assert sorted(losses) == ['loss_bbox', 'loss_centerness', 'loss_cls']
    for k, v in losses.items():
        assert np.allclose(v.item(), gold[f'{tag}_{k}'], rtol=1e-5, atol=1e-7), (k, v.item(), gold[f'{tag}_{k}'])
    sum(losses.values()).backward()
    assert all(torch.isfinite(t.grad).all() for t in cls + raw + ctr)
    if C == 4:
        for l in range(len(fi.SIZES)):
            for name, t in (('dcls', cls), ('dreg', raw), ('dctr', ctr)):
                assert np.allclose(t[l].grad.numpy(), gold[f'{tag}_{name}{l}'], rtol=1e-4, atol=1e-8), (name, l)
        assert np.allclose(torch.stack([s.grad for s in scales]).numpy(), gold[f'{tag}_dscale'], rtol=1e-4, atol=1e-8)


def test_loss_host_mirror_without_ground_truth():
    head = build(4, True)
    cls, raw, ctr = fi.head_outputs(5, grad=True)
    empty = [torch.zeros(0, 4), torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.long)] * 2
    losses = head.loss(cls, fi.decoded(raw, fi.SCALES, False, True), ctr, *empty, fi.metas())
    assert float(losses['loss_bbox']) == 0 and float(losses['loss_centerness']) == 0 and float(losses['loss_cls']) > 0


# ------------------------------------------------------------------------------------------- float64 restatement pinned
@pytest.mark.parametrize('tag', list(TARGET_CASES))
def test_float64_assignment_agrees_with_the_fixture(gold, tag):
    """the restated assignment gives the reference's label map, evaluated in float32 (the reference's own comparisons)
    and in float64 (no decision of these inputs sits on a rounding edge)"""
    seed = int(gold['seed_targets'])
    gt_bboxes, gt_labels = fi.gts(seed)
    over = TARGET_CASES[tag]
    for dtype in (torch.float32, torch.float64):
        inds = R.assign(gt_bboxes, fi.SIZES, fi.STRIDES, fi.RANGES, over.get('center_sampling', False),
                        over.get('center_sample_radius', 1.5), dtype)
        n_l = [h * w for h, w in fi.SIZES]
        for l in range(len(fi.SIZES)):
            got = torch.cat([torch.where(inds[b] >= 0, gt_labels[b][inds[b].clamp(min=0)], torch.tensor(4)).split(n_l)[l]
                             for b in range(2)])
            assert np.array_equal(got.numpy(), gold[f'targets_{tag}_labels{l}']), (tag, l, dtype)


@pytest.mark.parametrize('variant,C', [(v, c) for v in fi.VARIANTS for c in (4, 1)])
def test_float64_loss_agrees_with_the_fixture(gold, variant, C):
    """the fixture is ONE fp32 evaluation of the same sums, by torch on the CPU: a few dozen positive terms and 2048 x C
    focal terms, each a handful of roundings, summed pairwise.  64 eps of the value covers that (the same order as the
    rtol of 1e-5 the host mirror is held to above); the float64 gradients agree with the reference's autograd gradients
    to 1e-4 of the largest gradient of their tensor"""
    tag = f'loss_{variant}_c{C}'
    seed = int(gold[f'seed_{tag}'])
    over = fi.VARIANTS[variant]
    norm, giou = bool(over.get('norm_on_bbox', False)), variant == 'giou'
    cls, raw, ctr = fi.head_outputs(seed, C, norm_on_bbox=norm)
    gt_bboxes, gt_labels = fi.gts(seed, num_classes=C)
    inds = R.assign(gt_bboxes, fi.SIZES, fi.STRIDES, fi.RANGES, over.get('center_sampling', False),
                    over.get('center_sample_radius', 1.5), torch.float32)
    ref = R.loss(cls, raw, ctr, fi.SCALES, inds, gt_bboxes, gt_labels, fi.SIZES, fi.STRIDES, norm, giou)
    assert ref['n_pos'] > 5
    if norm:
        assert (ref['scaled'] < 0).any()            # the relu branch runs
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness')):
        want = float(gold[f'{tag}_{k}'])
        assert abs(float(ref['losses'][i]) - want) <= 64 * EPS32 * abs(want), (k, float(ref['losses'][i]), want)
    if C == 4:
        for l in range(len(fi.SIZES)):
            for name, key in (('dcls', 'dcls'), ('dreg', 'draw'), ('dctr', 'dctr')):
                g = gold[f'{tag}_{name}{l}'].astype(np.float64)
                assert np.abs(ref[key][l].numpy() - g).max() <= 1e-4 * max(np.abs(g).max(), 1e-12), (name, l)
        g = gold[f'{tag}_dscale'].astype(np.float64)
        assert np.abs(ref['dscale'].numpy() - g).max() <= 1e-4 * np.abs(g).max()
