"""CPU tests (-m "not gpu") of the VFNet baseline: the recipe builds and equals the reference's (the resolved reference recipe
is a section of the fixture), its parameters are the reference's, the refused settings raise with their names, the torch host
mirrors of VFNetHead.forward / get_targets / loss / get_bboxes reproduce what the reference computed
(tests/golden/g31_vfnet.npz, made by tests/golden/make_golden_vfnet.py), and the float64 restatement (tests/vfnet_ref64.py) is
pinned to the fixture before the GPU tests lean on it.  Tolerances are those tests/test_gfl_cpu.py uses for the same kinds of
quantity."""
import json
import math
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, build_head
from brcnn.config import ConfigDict
from oracle import orc
from tests import atss_ref64 as RA
from tests import vfnet_inputs as vi
from tests import vfnet_ref64 as R

G = os.path.join(os.path.dirname(__file__), 'golden', 'g31_vfnet.npz')
EPS32 = float(np.finfo(np.float32).eps)
L = len(vi.SIZES)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(vi.CONFIG).model)


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(vi.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, vi.SCALES):
            s.scale.fill_(v)
        for s, v in zip(head.scales_refine, vi.SCALES_REFINE):
            s.scale.fill_(v)
    return head


def test_config_builds_the_baseline(model):
    from brcnn.core import ATSSAssigner
    from brcnn.dense_heads import ATSSHead, DeformConv2d, GFLHead, GNTowerHead, VFNetHead
    from brcnn.detectors import VFNet, SingleStageDetector
    from brcnn.losses import GIoULoss, VarifocalLoss
    from brcnn.necks import FPN
    from brcnn.registry import DETECTORS, HEADS, LOSSES
    assert HEADS.get('VFNetHead') is VFNetHead and DETECTORS.get('VFNet') is VFNet
    assert LOSSES.get('VarifocalLoss') is VarifocalLoss
    assert type(model) is VFNet and isinstance(model, SingleStageDetector)
    assert type(model.bbox_head) is VFNetHead and type(model.neck) is FPN and model.neck.relu_before_extra_convs
    h = model.bbox_head
    assert isinstance(h, GNTowerHead) and not isinstance(h, (ATSSHead, GFLHead))          # beside ATSS and GFL, below neither
    assert h.cls_out_channels == 4 and h.strides == vi.STRIDES and h.stacked_convs == 3 and h.num_anchors == 1
    assert h.reg_denoms == vi.REG_DENOMS and h.gradient_mul == 0.1 and h.bbox_norm_type == 'reg_denom'
    assert type(h.assigner) is ATSSAssigner and h.assigner.topk == 9
    assert type(h.loss_cls) is VarifocalLoss and (h.loss_cls.alpha, h.loss_cls.gamma, h.loss_cls.iou_weighted) == (0.75, 2.0, True)
    assert type(h.loss_bbox) is GIoULoss and h.loss_bbox.loss_weight == 1.5
    assert type(h.loss_bbox_refine) is GIoULoss and h.loss_bbox_refine.loss_weight == 2.0
    assert type(h.vfnet_cls_dconv) is DeformConv2d and type(h.vfnet_reg_refine_dconv) is DeformConv2d
    assert [tuple(b.tolist()[0]) for b in h.anchor_generator.base_anchors][0] == (-32.0, -32.0, 32.0, 32.0)     # centre offset 0
    assert h.test_cfg.nms_pre == 1000 and h.test_cfg.max_per_img == 100 and h.test_cfg.nms.iou_threshold == 0.6
    assert not model.with_rpn and not model.with_roi_head and not h.supports_tta
    h._check_limits(h.test_cfg, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])       # the recipe's sizes (800 x 1344)
    assert 'configs/vfnet' in open(os.path.join(vi.ROOT, 'tools', 'bench_recipes.py')).read()


def test_shipped_config_equals_the_reference_config(gold):
    """the shipped rewrite equals, key for key, what the reference recipe resolves to through this repo's loader (recorded in
    the fixture by the generator)"""
    want = json.loads(str(gold['config_json']))
    assert want['model']['type'] == 'VFNet' and want['model']['bbox_head']['num_classes'] == 4
    got = json.loads(json.dumps(Config.fromfile(vi.CONFIG).to_dict(), sort_keys=True))
    assert got == want


def test_parameter_names_and_shapes_are_the_references(model, gold):
    sd = model.state_dict()
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want
    assert list(sd) == [str(k) for k in gold['state_keys']]
    fresh = build_detector(Config.fromfile(vi.CONFIG).model)
    res = fresh.load_state_dict({str(k): torch.zeros(json.loads(str(s))) for k, s in zip(gold['state_keys'], gold['state_shapes'])})
    assert not res.missing_keys and not res.unexpected_keys
    h = build_head(ConfigDict(vi.head_cfg(num_classes=3, in_channels=16, feat_channels=32, stacked_convs=1)))
    assert [k for k in h.state_dict()] == [
        'cls_convs.0.conv.weight', 'cls_convs.0.gn.weight', 'cls_convs.0.gn.bias',
        'reg_convs.0.conv.weight', 'reg_convs.0.gn.weight', 'reg_convs.0.gn.bias',
        'vfnet_reg_conv.conv.weight', 'vfnet_reg_conv.gn.weight', 'vfnet_reg_conv.gn.bias', 'vfnet_reg.weight', 'vfnet_reg.bias',
        'scales.0.scale', 'scales.1.scale', 'scales.2.scale', 'scales.3.scale', 'scales.4.scale',
        'vfnet_reg_refine_dconv.weight', 'vfnet_reg_refine.weight', 'vfnet_reg_refine.bias',
        'scales_refine.0.scale', 'scales_refine.1.scale', 'scales_refine.2.scale', 'scales_refine.3.scale', 'scales_refine.4.scale',
        'vfnet_cls_dconv.weight', 'vfnet_cls.weight', 'vfnet_cls.bias']
    assert h.vfnet_cls.weight.shape == (3, 32, 3, 3) and h.vfnet_reg.weight.shape == (4, 32, 3, 3)
    assert h.vfnet_cls_dconv.weight.shape == (32, 32, 3, 3) and h.vfnet_reg_refine_dconv.weight.shape == (32, 32, 3, 3)
    # Normal(0, 0.01) convs, zero biases but vfnet_cls's, which starts at the prior 0.01; the deformable convs keep
    # kaiming-uniform (they are no Conv2d): bound sqrt(6 / fan_in) = sqrt(6 / 288) = 0.144
    assert torch.allclose(h.vfnet_cls.bias, torch.full((3,), -float(np.log(99.0))))
    assert float(h.vfnet_reg.bias.detach().abs().max()) == 0 and 0.005 < float(h.vfnet_reg_conv.conv.weight.detach().std()) < 0.02
    assert 0.12 < float(h.vfnet_cls_dconv.weight.detach().abs().max()) <= math.sqrt(6 / 288) + 1e-6


def _ag(**kw):
    return dict(dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=2, scales_per_octave=1, center_offset=0.0,
                     strides=vi.STRIDES), **kw)


def _tc(**kw):
    return dict(dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False), **kw)


VFL = dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True, loss_weight=1.0)
REFUSED = [
    (dict(use_atss=False), NotImplementedError, 'use_atss'),
    (dict(use_vfl=False), NotImplementedError, 'use_vfl'),
    (dict(dcn_on_last_conv=True), NotImplementedError, 'dcn_on_last_conv'),
    (dict(sync_num_pos=False), NotImplementedError, 'sync_num_pos'),
    (dict(feat_channels=512, in_channels=512), NotImplementedError, 'feat_channels'),
    (dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0)), NotImplementedError, 'loss_cls'),
    (dict(loss_cls=dict(VFL, use_sigmoid=False)), NotImplementedError, 'loss_cls'),
    (dict(loss_cls=dict(VFL, gamma=0.5)), NotImplementedError, 'gamma'),
    (dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)), NotImplementedError, 'loss_bbox'),
    (dict(loss_bbox_refine=dict(type='L1Loss', loss_weight=1.0)), NotImplementedError, 'loss_bbox_refine'),
    (dict(loss_cls=dict(VFL, reduction='sum')), NotImplementedError, 'reduction'),
    (dict(loss_bbox=dict(type='GIoULoss', reduction='sum')), NotImplementedError, 'reduction'),
    (dict(loss_bbox_refine=dict(type='GIoULoss', reduction='none')), NotImplementedError, 'reduction'),
    (dict(norm_cfg=None), NotImplementedError, 'norm_cfg'),
    (dict(norm_cfg=dict(type='BN', requires_grad=True)), NotImplementedError, 'norm_cfg'),
    (dict(anchor_generator=_ag(ratios=[0.5, 1.0])), NotImplementedError, 'anchors per cell'),
    (dict(anchor_generator=_ag(scales_per_octave=2)), NotImplementedError, 'scales_per_octave'),
    (dict(anchor_generator=_ag(strides=[(8, 16), (16, 16), (32, 32), (64, 64), (128, 128)])), NotImplementedError, 'square strides'),
    (dict(train_cfg=_tc(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4))), NotImplementedError, 'assigner'),
    (dict(train_cfg=_tc(assigner=dict(type='ATSSAssigner', topk=9, ignore_iof_thr=0.5))), NotImplementedError, 'ignore_iof_thr'),
    (dict(train_cfg=_tc(pos_weight=2.0)), NotImplementedError, 'pos_weight'),
    (dict(train_cfg=_tc(allowed_border=0)), NotImplementedError, 'allowed_border'),
    (dict(test_cfg=dict(vi.TEST_CFG, nms=dict(type='soft_nms', iou_threshold=0.5))), NotImplementedError, 'soft'),
    (dict(test_cfg=dict(vi.TEST_CFG, nms=dict(type='nms', iou_threshold=0.5, class_agnostic=True))), NotImplementedError,
     'class_agnostic'),
    (dict(feat_channels=66, norm_cfg=dict(type='GN', num_groups=2, requires_grad=True)), NotImplementedError, 'feat_channels'),
    (dict(bbox_norm_type='area'), NotImplementedError, 'bbox_norm_type'),
    (dict(strides=[4, 8, 16, 32, 64]), ValueError, 'strides'),
]


@pytest.mark.parametrize('over,exc,name', REFUSED, ids=[f'{i}-{n}' for i, (_, _, n) in enumerate(REFUSED)])
def test_refused_settings_raise_with_their_name(over, exc, name):
    with pytest.raises(exc, match=name):
        build_head(ConfigDict(vi.head_cfg(**over)))


def test_refused_calls_raise_with_their_name(model):
    head = build()
    cls, raw0, raw1 = vi.head_outputs(3)
    d0, d1 = vi.distances(raw0, raw1)
    with pytest.raises(NotImplementedError, match='with_nms=False'):
        head.get_bboxes(cls, d0, d1, vi.metas(), with_nms=False)
    with pytest.raises(NotImplementedError, match='gt_bboxes_ignore'):
        head.forward_train_nhwc(None, vi.metas(), None, None, gt_bboxes_ignore=[torch.zeros(0, 4)] * 2)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(vi.TEST_CFG, nms_pre=5000), vi.SIZES)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(vi.TEST_CFG, nms_pre=-1), vi.SIZES)
    # the 16-bit deformable kernels take channels in eights: a head of 68 channels builds (fp32 takes quads) and is refused
    # where a 16-bit map reaches the star convs
    h68 = build_head(ConfigDict(vi.head_cfg(feat_channels=68, norm_cfg=dict(type='GN', num_groups=2, requires_grad=True))))
    h68._check_dcn_channels(torch.zeros(1))
    with pytest.raises(NotImplementedError, match='feat_channels'):
        h68._check_dcn_channels(torch.zeros(1, dtype=torch.bfloat16))
    imgs = [torch.zeros(1, 3, vi.H, vi.W), torch.zeros(1, 3, vi.H, vi.W)]
    metas = [vi.metas(1), [dict(vi.metas(1)[0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.forward_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        head.aug_test(None, metas)


# ------------------------------------------------------------------------------------------- pieces by hand
def test_star_offsets_by_hand():
    """raw = 0, scale = 1, level 0: D0 = 64 exactly, 8 cells; tap 0 (top-left corner) moves by (-8, -8) - (-1, -1), the
    centre tap not at all, tap 8 by (8, 8) - (1, 1)"""
    head = build()
    d0 = torch.full((1, 4, 2, 3), 64.0)
    off = head.star_dcn_offset(d0, 0.1, 8)
    assert off.shape == (1, 18, 2, 3)
    o = off[0, :, 0, 0].tolist()
    assert o[0:2] == [-7.0, -7.0] and o[8:10] == [0.0, 0.0] and o[16:18] == [7.0, 7.0]
    assert o[2:4] == [-7.0, 0.0] and o[6:8] == [0.0, -7.0] and o[10:12] == [0.0, 7.0] and o[14:16] == [7.0, 0.0]
    assert o[4:6] == [-7.0, 7.0] and o[12:14] == [7.0, -7.0]
    ref = R.star_offsets(torch.full((4,), 64.0, dtype=torch.float64), 0.1, 8)
    assert np.allclose(ref.numpy(), o, rtol=0, atol=1e-12)
    # the gradient reaches the distances through the gradient_mul share only: d (-top / 8) = -0.1 / 8 on three entries
    d = torch.full((4,), 64.0, dtype=torch.float64, requires_grad=True)
    R.star_offsets(d, 0.1, 8).sum().backward()
    assert np.allclose(d.grad.numpy(), [-3 * 0.1 / 8, -3 * 0.1 / 8, 3 * 0.1 / 8, 3 * 0.1 / 8], rtol=1e-12)


def test_host_deform_conv_against_the_restatement_and_a_plain_conv():
    from brcnn.dense_heads import deform_conv2d_host
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 6, 7, generator=g, dtype=torch.float64)
    w = torch.randn(5, 8, 3, 3, generator=g, dtype=torch.float64)
    zero = torch.zeros(2, 18, 6, 7, dtype=torch.float64)
    plain = torch.nn.functional.conv2d(x, w, padding=1)
    assert np.allclose(deform_conv2d_host(x, zero, w).numpy(), plain.numpy(), rtol=1e-12, atol=1e-12)
    off = (torch.randn(2, 18, 6, 7, generator=g, dtype=torch.float64) * 3).requires_grad_()
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = deform_conv2d_host(xg, off, wg)
    y2 = R.deform_conv_v1(x.permute(0, 2, 3, 1), off.detach().permute(0, 2, 3, 1), w).permute(0, 3, 1, 2)
    assert np.allclose(y.detach().numpy(), y2.numpy(), rtol=1e-12, atol=1e-12)
    y.square().sum().backward()
    o2, x2, w2 = (off.detach().permute(0, 2, 3, 1).clone().requires_grad_(), x.permute(0, 2, 3, 1).clone().requires_grad_(),
                  w.clone().requires_grad_())
    R.deform_conv_v1(x2, o2, w2).square().sum().backward()
    assert np.allclose(off.grad.permute(0, 2, 3, 1).numpy(), o2.grad.numpy(), rtol=1e-10, atol=1e-10)
    assert np.allclose(xg.grad.permute(0, 2, 3, 1).numpy(), x2.grad.numpy(), rtol=1e-10, atol=1e-10)
    assert np.allclose(wg.grad.numpy(), w2.grad.numpy(), rtol=1e-10, atol=1e-10)
    # a sample beyond (-1, H) x (-1, W) is zero: far offsets on every tap leave nothing
    far = torch.full((2, 18, 6, 7), 1e6, dtype=torch.float64)
    assert float(deform_conv2d_host(x, far, w).abs().max()) == 0
    assert float(deform_conv2d_host(x, far * float('inf'), w).abs().max()) == 0


# ------------------------------------------------------------------------------------------- host mirror vs the fixture
def test_get_targets_host_mirror_is_exact(gold):
    head = build(4, True)
    seed = int(gold['seed_targets'])
    gt_bboxes, gt_labels = vi.gts(seed)
    cls, _, _ = vi.head_outputs(seed)
    pts = head.get_points(vi.SIZES, torch.float32, 'cpu')
    labels, _, targets, _ = head.get_targets(cls, pts, gt_bboxes, gt_labels, vi.metas(), None)
    for l in range(L):
        assert np.array_equal(labels[l].numpy(), gold[f'targets_labels{l}']), l
        assert np.array_equal(targets[l].numpy(), gold[f'targets_ltrb{l}']), l
    assert sum(bool((labels[l] < 4).any()) for l in range(L)) >= 3


@pytest.mark.parametrize('tag,C,pads', [('loss_c4', 4, None), ('loss_c1', 1, None), ('loss_pad', 4, [(128, 192), (96, 160)])])
def test_loss_host_mirror_reproduces_the_reference(gold, tag, C, pads):
    seed = int(gold[f'seed_{tag}'])
    head = build(C, True)
    cls, raw0, raw1 = vi.head_outputs(seed, C)
    d0, d1 = vi.distances(raw0, raw1)
    cls, d0, d1 = ([t.detach().requires_grad_() for t in lst] for lst in (cls, d0, d1))
    gt_bboxes, gt_labels = vi.gts(seed, num_classes=C)
    losses = head.loss(cls, d0, d1, gt_bboxes, gt_labels, vi.metas(pads=pads))
    assert sorted(losses) == ['loss_bbox', 'loss_bbox_rf', 'loss_cls']
    for k, v in losses.items():
        assert np.allclose(float(v.detach()), gold[f'{tag}_{k}'], rtol=1e-5, atol=1e-7), (k, float(v.detach()), gold[f'{tag}_{k}'])
    sum(losses.values()).backward()
    assert all(torch.isfinite(t.grad).all() for t in cls + d0 + d1)
    if tag == 'loss_c4':
        for l in range(L):
            for name, t in (('dcls', cls), ('dd0', d0), ('dd1', d1)):
                assert np.allclose(t[l].grad.numpy(), gold[f'{tag}_{name}{l}'], rtol=1e-4, atol=1e-8), (name, l)


def test_invalid_cells_count_as_background(gold):
    """the two sections share their seed: only pad_shape (and with it the assignment) differs, and the class loss with it"""
    assert int(gold['seed_loss_pad']) == int(gold['seed_loss_c4'])
    assert abs(float(gold['loss_pad_loss_cls']) - float(gold['loss_c4_loss_cls'])) > 1e-3 * float(gold['loss_c4_loss_cls'])


def test_loss_host_mirror_without_ground_truth():
    head = build(4, True)
    cls, raw0, raw1 = vi.head_outputs(5, grad=True)
    d0, d1 = vi.distances(raw0, raw1)
    empty = [torch.zeros(0, 4), torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.long)] * 2
    losses = head.loss(cls, d0, d1, *empty, vi.metas())
    assert losses['loss_bbox'].item() == 0 and losses['loss_bbox_rf'].item() == 0 and losses['loss_cls'].item() > 0


CASES = [(4, 'plain'), (4, 'rescale'), (4, 'empty'), (1, 'plain'), (1, 'rescale')]


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_host_mirror_reproduces_the_reference(gold, C, name):
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C)
    cls, raw0, raw1 = vi.head_outputs(seed, C, empty=(name == 'empty'))
    d0, d1 = vi.distances(raw0, raw1)
    res = head.get_bboxes(cls, d0, d1, vi.metas(), rescale=(name != 'plain'), batched_nms=orc.batched_nms)
    for b, (det, lab) in enumerate(res):
        want_d, want_l = gold[f'bboxes_c{C}_{name}_det{b}'], gold[f'bboxes_c{C}_{name}_lab{b}']
        assert lab.tolist() == want_l.tolist(), (C, name, b)
        assert det.shape == want_d.shape and np.allclose(det.numpy(), want_d, rtol=0, atol=1e-5), (C, name, b)
    if name == 'empty':
        assert len(res[1][0]) == 0 and len(res[0][0]) > 0


def test_forward_host_mirror_reproduces_the_reference(gold):
    """class logits and both distances through the star deformable convs; the distances are exp() of a conv output times up
    to 1024, so they are compared relatively"""
    seed = int(gold['seed_forward'])
    head = build(4)
    head.load_state_dict(vi.seeded_head_state(head, seed))
    with torch.no_grad():
        cls, d0, d1 = head(vi.features(seed))
    assert [tuple(c.shape) for c in cls] == [(2, 4, h, w) for h, w in vi.SIZES] and d0[0].dtype == torch.float32
    for l in range(L):
        assert np.allclose(cls[l].numpy(), gold[f'fwd_cls{l}'], rtol=1e-4, atol=1e-5), l
        assert np.allclose(d0[l].numpy(), gold[f'fwd_d0{l}'], rtol=1e-5, atol=0), l
        assert np.allclose(d1[l].numpy(), gold[f'fwd_d1{l}'], rtol=1e-4, atol=0), l
    # the conditioning: first distances near reg_denom, 8 cells -- inside the 16 x 24 map, far outside the 1 x 2 one
    assert 30 < float(d0[0].mean()) < 100 and 500 < float(d0[4].mean()) < 1600


def test_forward_gradient_through_the_offsets(gold):
    seed = int(gold['seed_forward_grad'])
    head = build(4)
    head.load_state_dict(vi.seeded_head_state(head, seed))
    x = vi.small_feature(seed).requires_grad_()
    cls, d0, d1 = head([x])
    off = head.star_dcn_offset(d0[0].detach().double(), vi.GRADIENT_MUL, vi.STRIDES[0]).permute(0, 2, 3, 1)
    assert R.integer_margin(off) > 1e-3                                           # the generator's condition
    (cls[0].sum() + d1[0].log().sum()).backward()
    assert np.allclose(cls[0].detach().numpy(), gold['fgrad_cls'], rtol=1e-4, atol=1e-5)
    assert np.allclose(d1[0].detach().numpy(), gold['fgrad_d1'], rtol=1e-4, atol=0)
    g = gold['fgrad_dx']
    assert np.abs(x.grad.numpy() - g).max() <= 1e-4 * np.abs(g).max()


# ------------------------------------------------------------------------------------------- float64 restatement pinned
@pytest.mark.parametrize('tag,C,pads', [('loss_c4', 4, None), ('loss_c1', 1, None), ('loss_pad', 4, [(128, 192), (96, 160)])])
def test_float64_loss_agrees_with_the_fixture(gold, tag, C, pads):
    """the fixture is ONE fp32 evaluation of the same sums, by torch on the CPU: up to 1024 x C class terms and a few dozen
    positive terms, each a handful of roundings, summed pairwise: 64 eps of the value, as tests/test_gfl_cpu.py allows.  The
    float64 gradients agree with the reference's autograd gradients to 1e-4 of the largest gradient of their tensor"""
    seed = int(gold[f'seed_{tag}'])
    cls, raw0, raw1 = vi.head_outputs(seed, C)
    d0, d1 = vi.distances(raw0, raw1)
    gt_bboxes, gt_labels = vi.gts(seed, num_classes=C)
    valid = None if pads is None else [[[min(math.ceil(p[0] / s), h), min(math.ceil(p[1] / s), w)]
                                        for (h, w), s in zip(vi.SIZES, vi.STRIDES)] for p in pads]
    inds = RA.assign(gt_bboxes, vi.SIZES, vi.STRIDES, vi.OCTAVE, vi.TOPK, valid_hws=valid, dtype=torch.float32)
    ref = R.loss(cls, d0, d1, inds, gt_bboxes, gt_labels, vi.SIZES, vi.STRIDES)
    assert ref['n_pos'] > 5
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_bbox_rf')):
        want = float(gold[f'{tag}_{k}'])
        assert abs(float(ref['losses'][i]) - want) <= 64 * EPS32 * abs(want), (k, ref['losses'][i], want)
    if tag == 'loss_c4':
        for l in range(L):
            for name in ('dcls', 'dd0', 'dd1'):
                g = gold[f'{tag}_{name}{l}'].astype(np.float64)
                assert np.abs(ref[name][l].numpy() - g).max() <= 1e-4 * max(np.abs(g).max(), 1e-12), (name, l)


def test_float64_candidates_agree_with_the_host_mirror(gold):
    from brcnn.dense_heads import distance2bbox
    seed = int(gold['seed_bboxes_c4'])
    head = build(4)
    cls, raw0, raw1 = vi.head_outputs(seed, 4)
    _, d1 = vi.distances(raw0, raw1)
    metas = vi.metas()
    ref = R.candidates(cls, d1, vi.SIZES, vi.STRIDES, [m['img_shape'] for m in metas])
    for l, pts in enumerate(head.get_points(vi.SIZES, torch.float32, 'cpu')):
        for b in range(2):
            h, w = metas[b]['img_shape'][:2]
            want = distance2bbox(pts, d1[l][b].permute(1, 2, 0).reshape(-1, 4))
            want = torch.stack([want[:, 0].clamp(0, w), want[:, 1].clamp(0, h), want[:, 2].clamp(0, w), want[:, 3].clamp(0, h)], -1)
            assert np.allclose(ref[l][2][b].numpy(), want.numpy(), rtol=1e-6, atol=1e-3), (l, b)


def test_float64_forward_chain_agrees_with_the_fixture(gold):
    """the restated star chain (distances, offsets, DCN v1) on level 0 of the forward section, through the head's own towers"""
    seed = int(gold['seed_forward'])
    head = build(4).double()
    head.load_state_dict(vi.seeded_head_state(head, seed))
    feats = [f.double() for f in vi.features(seed)]
    import torch.nn.functional as F
    with torch.no_grad():
        for l in (0, 4):
            c, r = head._towers_host(feats[l])
            m = head.vfnet_reg_conv
            ri = F.relu(F.group_norm(F.conv2d(r, m.conv.weight, None, padding=1), m.norm.num_groups, m.norm.weight, m.norm.bias,
                                     m.norm.eps))
            raw0 = F.conv2d(ri, head.vfnet_reg.weight, head.vfnet_reg.bias, padding=1).permute(0, 2, 3, 1)
            scales = torch.stack([s.scale for s in head.scales])
            d0, off, yr, yc = R.star_chain([raw0], scales[l:l + 1], [r.permute(0, 2, 3, 1)], [c.permute(0, 2, 3, 1)],
                                           head.vfnet_reg_refine_dconv.weight, head.vfnet_cls_dconv.weight, vi.STRIDES[l:l + 1],
                                           vi.REG_DENOMS[l:l + 1], vi.GRADIENT_MUL)[0]
            assert np.allclose(d0.permute(0, 3, 1, 2).numpy(), gold[f'fwd_d0{l}'], rtol=1e-5, atol=0)
            cls = F.conv2d(yc.permute(0, 3, 1, 2), head.vfnet_cls.weight, head.vfnet_cls.bias, padding=1)
            assert np.allclose(cls.numpy(), gold[f'fwd_cls{l}'], rtol=1e-4, atol=1e-5)
