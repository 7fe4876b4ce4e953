"""CPU tests (-m "not gpu") of the ATSS baseline: the recipe builds and equals the reference's, its parameters are the
reference's, the refused settings raise with their names, the torch host mirrors of ATSSAssigner.assign and ATSSHead.get_targets
/ loss / get_bboxes reproduce what the reference computed (tests/golden/g29_atss.npz, made by
tests/golden/make_golden_atss.py), and the float64 restatement (tests/atss_ref64.py) is pinned to the fixture before the GPU
tests lean on it."""
import json
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, build_head
from brcnn.config import ConfigDict
from oracle import orc
from tests import atss_inputs as ai
from tests import atss_ref64 as R

G = os.path.join(os.path.dirname(__file__), 'golden', 'g29_atss.npz')
REF_CONFIG = '/root/reference/configs/atss/atss_r50_fpn_1x_coco.py'
EPS32 = float(np.finfo(np.float32).eps)
L = len(ai.SIZES)
N_L = [h * w for h, w in ai.SIZES]


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(ai.CONFIG).model)


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(ai.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, ai.SCALES):
            s.scale.fill_(v)
    return head


def grid(head):
    return head.anchor_generator.grid_anchors(ai.SIZES, 'cpu')


def test_config_builds_the_baseline(model):
    from brcnn.core import ATSSAssigner
    from brcnn.dense_heads import ATSSHead
    from brcnn.detectors import ATSS, SingleStageDetector
    from brcnn.necks import FPN
    from brcnn.registry import BBOX_ASSIGNERS, DETECTORS, HEADS
    assert HEADS.get('ATSSHead') is ATSSHead and DETECTORS.get('ATSS') is ATSS and BBOX_ASSIGNERS.get('ATSSAssigner') is ATSSAssigner
    assert type(model) is ATSS and isinstance(model, SingleStageDetector)
    assert type(model.bbox_head) is ATSSHead and type(model.neck) is FPN
    h = model.bbox_head
    assert h.cls_out_channels == 4 and h.strides == ai.STRIDES and h.stacked_convs == 4 and h.num_anchors == 1
    assert type(h.assigner) is ATSSAssigner and h.assigner.topk == 9 and h.assigner.ignore_iof_thr == -1
    assert [b.tolist() for b in h.anchor_generator.base_anchors] == [[[-4. * s, -4. * s, 4. * s, 4. * s]] for s in ai.STRIDES]
    assert tuple(h.bbox_coder.stds) == (0.1, 0.1, 0.2, 0.2) and tuple(h.bbox_coder.means) == (0., 0., 0., 0.)
    assert (h.loss_cls.gamma, h.loss_cls.alpha) == (2.0, 0.25) and type(h.loss_bbox).__name__ == 'GIoULoss'
    assert h.loss_bbox.loss_weight == 2.0 and h.loss_centerness.use_sigmoid
    assert h.test_cfg.nms_pre == 1000 and h.test_cfg.max_per_img == 100 and h.test_cfg.nms.iou_threshold == 0.6
    assert not model.with_rpn and not model.with_roi_head and not h.supports_tta
    h._check_limits(h.test_cfg, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])       # the recipe's sizes (800 x 1344)
    assert 'configs/atss' in open(os.path.join(ai.ROOT, 'tools', 'bench_recipes.py')).read()


@pytest.mark.skipif(not os.path.isfile(REF_CONFIG), reason='reference tree absent')
def test_shipped_config_equals_the_reference_config():
    """the reference recipe loads UNCHANGED through this repo's loader and equals the shipped rewrite key for key"""
    r = Config.fromfile(REF_CONFIG).to_dict()
    assert 'model' in r and r['model']['type'] == 'ATSS'
    assert Config.fromfile(ai.CONFIG).to_dict() == r


def test_parameter_names_and_shapes_are_the_references(model, gold):
    sd = model.state_dict()
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want
    assert list(sd) == [str(k) for k in gold['state_keys']]
    fresh = build_detector(Config.fromfile(ai.CONFIG).model)
    res = fresh.load_state_dict({str(k): torch.zeros(json.loads(str(s))) for k, s in zip(gold['state_keys'], gold['state_shapes'])})
    assert not res.missing_keys and not res.unexpected_keys
    h = build_head(ConfigDict(ai.head_cfg(num_classes=3, in_channels=16, feat_channels=32, stacked_convs=1)))
    assert [k for k in h.state_dict()] == [
        'cls_convs.0.conv.weight', 'cls_convs.0.gn.weight', 'cls_convs.0.gn.bias',
        'reg_convs.0.conv.weight', 'reg_convs.0.gn.weight', 'reg_convs.0.gn.bias',
        'atss_cls.weight', 'atss_cls.bias', 'atss_reg.weight', 'atss_reg.bias', 'atss_centerness.weight',
        'atss_centerness.bias', 'scales.0.scale', 'scales.1.scale', 'scales.2.scale', 'scales.3.scale', 'scales.4.scale']
    assert h.atss_cls.weight.shape == (3, 32, 3, 3) and h.atss_reg.weight.shape == (4, 32, 3, 3)
    assert h.atss_centerness.weight.shape == (1, 32, 3, 3) and h.scales[0].scale.shape == ()
    # Normal(0, 0.01) convs, zero biases but atss_cls's, which starts at the prior 0.01
    assert torch.allclose(h.atss_cls.bias, torch.full((3,), -float(np.log(99.0))))
    assert float(h.atss_reg.bias.detach().abs().max()) == 0 and 0.005 < float(h.cls_convs[0].conv.weight.detach().std()) < 0.02


def _ag(**kw):
    return dict(dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=2, scales_per_octave=1, strides=ai.STRIDES), **kw)


def _tc(**kw):
    return dict(dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False), **kw)


REFUSED = [
    (dict(anchor_generator=_ag(ratios=[0.5, 1.0])), NotImplementedError, 'anchors per cell'),
    (dict(anchor_generator=_ag(scales_per_octave=2)), NotImplementedError, 'scales_per_octave'),
    (dict(norm_cfg=None), NotImplementedError, 'norm_cfg'),
    (dict(norm_cfg=dict(type='BN', requires_grad=True)), NotImplementedError, 'norm_cfg'),
    (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)), NotImplementedError, 'use_sigmoid=False'),
    (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)), NotImplementedError, 'loss_cls'),
    (dict(loss_bbox=dict(type='L1Loss', loss_weight=1.0)), NotImplementedError, 'loss_bbox'),
    (dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)), NotImplementedError, 'loss_bbox'),
    (dict(loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)), NotImplementedError, 'loss_centerness'),
    (dict(loss_centerness=dict(type='MSELoss', loss_weight=1.0)), NotImplementedError, 'loss_centerness'),
    (dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, reduction='sum')), NotImplementedError, 'reduction'),
    (dict(loss_bbox=dict(type='GIoULoss', reduction='sum')), NotImplementedError, 'reduction'),
    (dict(reg_decoded_bbox=True), NotImplementedError, 'reg_decoded_bbox=True'),
    (dict(train_cfg=_tc(pos_weight=2.0)), NotImplementedError, 'pos_weight'),
    (dict(train_cfg=_tc(allowed_border=0)), NotImplementedError, 'allowed_border'),
    (dict(train_cfg=_tc(assigner=dict(type='ATSSAssigner', topk=9, ignore_iof_thr=0.5))), NotImplementedError, 'ignore_iof_thr'),
    (dict(train_cfg=_tc(assigner=dict(type='ATSSAssigner', topk=17))), ValueError, 'topk'),
    (dict(train_cfg=_tc(assigner=dict(type='ATSSAssigner', topk=0))), ValueError, 'topk'),
    (dict(test_cfg=dict(ai.TEST_CFG, nms=dict(type='soft_nms', iou_threshold=0.5))), NotImplementedError, 'soft'),
    (dict(test_cfg=dict(ai.TEST_CFG, nms=dict(type='nms', iou_threshold=0.5, class_agnostic=True))), NotImplementedError,
     'class_agnostic'),
]


@pytest.mark.parametrize('over,exc,name', REFUSED, ids=[f'{i}-{n}' for i, (_, _, n) in enumerate(REFUSED)])
def test_refused_settings_raise_with_their_name(over, exc, name):
    with pytest.raises(exc, match=name):
        build_head(ConfigDict(ai.head_cfg(**over)))


def test_refused_calls_raise_with_their_name(model):
    head = build()
    cls, raw, ctr = ai.head_outputs(3)
    with pytest.raises(NotImplementedError, match='with_nms=False'):
        head.get_bboxes(cls, ai.scaled(raw, ai.SCALES), ctr, ai.metas(), with_nms=False)
    with pytest.raises(NotImplementedError, match='gt_bboxes_ignore'):
        head.forward_train_nhwc(None, ai.metas(), None, None, gt_bboxes_ignore=[torch.zeros(0, 4)] * 2)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(ai.TEST_CFG, nms_pre=5000), ai.SIZES)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(ai.TEST_CFG, nms_pre=-1), ai.SIZES)
    imgs = [torch.zeros(1, 3, ai.H, ai.W), torch.zeros(1, 3, ai.H, ai.W)]
    metas = [ai.metas(1), [dict(ai.metas(1)[0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.forward_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        head.aug_test(None, metas)


def test_the_rpn_head_still_refuses_atss_targets():
    from brcnn.dense_heads import ATSSRPNHead
    import inspect
    assert "assert not atss, 'atss=True (ATSSAssigner targets) is outside the shipped boosting configs'" in \
        inspect.getsource(ATSSRPNHead)


# ------------------------------------------------------------------------------------------- host mirror vs the fixture
def test_assigner_host_mirror_is_exact(gold):
    head = build(4, True)
    gt_bboxes, gt_labels = ai.gts(int(gold['seed_assign']))
    anchors = grid(head)
    for b in range(2):
        res = head.assigner.assign(torch.cat(anchors), [len(a) for a in anchors], gt_bboxes[b], None, gt_labels[b])
        assert np.array_equal(res.gt_inds.numpy(), gold[f'assign_gt_inds{b}']), b
        assert np.array_equal(res.labels.numpy(), gold[f'assign_labels{b}']), b
        assert np.array_equal(res.max_overlaps.numpy(), gold[f'assign_max_overlaps{b}']), b
        assert (res.gt_inds > 0).sum() > 5
    # any boxes, any number per cell: 5-column boxes in two "levels", no ground truth
    res = head.assigner.assign(torch.rand(7, 5), [4, 3], torch.zeros(0, 4), None, torch.zeros(0, dtype=torch.long))
    assert res.gt_inds.tolist() == [0] * 7 and res.labels.tolist() == [-1] * 7


def test_get_targets_host_mirror_is_exact(gold):
    head = build(4, True)
    gt_bboxes, gt_labels = ai.gts(int(gold['seed_targets']))
    anchor_list, valid_flag_list = head.get_anchors(ai.SIZES, ai.metas(), device='cpu')
    out = head.get_targets(anchor_list, valid_flag_list, gt_bboxes, ai.metas(), gt_labels_list=gt_labels, label_channels=4)
    _, labels, weights, targets, _, num_pos, num_neg = out
    for l in range(L):
        assert np.array_equal(labels[l].numpy(), gold[f'targets_labels{l}']), l
        assert np.array_equal(weights[l].numpy(), gold[f'targets_weights{l}']), l
        assert np.allclose(targets[l].numpy(), gold[f'targets_box{l}'], rtol=1e-6, atol=1e-6), l
    assert [num_pos, num_neg] == gold['targets_num'].tolist()
    assert sum(bool((labels[l] < 4).any()) for l in range(L)) >= 3


@pytest.mark.parametrize('C', [4, 1])
def test_loss_host_mirror_reproduces_the_reference(gold, C):
    tag = f'loss_c{C}'
    seed = int(gold[f'seed_{tag}'])
    head = build(C, True)
    cls, raw, ctr = ai.head_outputs(seed, C, grad=True)
    scales = [torch.tensor(v, requires_grad=True) for v in ai.SCALES]
    gt_bboxes, gt_labels = ai.gts(seed, num_classes=C)
    losses = head.loss(cls, ai.scaled(raw, scales), ctr, gt_bboxes, gt_labels, ai.metas())
    assert sorted(losses) == ['loss_bbox', 'loss_centerness', 'loss_cls']
    for k, v in losses.items():
        got = torch.stack([torch.as_tensor(x) for x in v]).detach().numpy()
        assert len(v) == L and np.allclose(got, gold[f'{tag}_{k}'], rtol=1e-5, atol=1e-7), (k, got, gold[f'{tag}_{k}'])
    sum(sum(v) for v in losses.values()).backward()
    assert all(torch.isfinite(t.grad).all() for t in cls + raw + ctr)
    if C == 4:
        for l in range(L):
            for name, t in (('dcls', cls), ('dreg', raw), ('dctr', ctr)):
                assert np.allclose(t[l].grad.numpy(), gold[f'{tag}_{name}{l}'], rtol=1e-4, atol=1e-8), (name, l)
        assert np.allclose(torch.stack([s.grad for s in scales]).numpy(), gold[f'{tag}_dscale'], rtol=1e-4, atol=1e-8)


def test_loss_host_mirror_without_ground_truth():
    head = build(4, True)
    cls, raw, ctr = ai.head_outputs(5, grad=True)
    empty = [torch.zeros(0, 4), torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.long)] * 2
    losses = head.loss(cls, ai.scaled(raw, ai.SCALES), ctr, *empty, ai.metas())
    assert all(x.item() == 0 for x in losses['loss_bbox']) and all(x.item() == 0 for x in losses['loss_centerness'])
    assert sum(losses['loss_cls']).item() > 0


CASES = [(4, 'plain'), (4, 'rescale'), (4, 'empty'), (1, 'plain'), (1, 'rescale')]


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_host_mirror_reproduces_the_reference(gold, C, name):
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C)
    cls, raw, ctr = ai.head_outputs(seed, C, empty=(name == 'empty'))
    res = head.get_bboxes(cls, ai.scaled(raw, ai.SCALES), ctr, ai.metas(), rescale=(name != 'plain'),
                          batched_nms=orc.batched_nms)
    for b, (det, lab) in enumerate(res):
        want_d, want_l = gold[f'bboxes_c{C}_{name}_det{b}'], gold[f'bboxes_c{C}_{name}_lab{b}']
        assert lab.tolist() == want_l.tolist(), (C, name, b)
        assert det.shape == want_d.shape and np.allclose(det.numpy(), want_d, rtol=0, atol=1e-5), (C, name, b)
    if name == 'empty':
        assert len(res[1][0]) == 0 and len(res[0][0]) > 0


# ------------------------------------------------------------------------------------------- float64 restatement pinned
def test_float64_anchors_are_the_generators():
    head = build()
    for a, b in zip(grid(head), R.anchors(ai.SIZES, ai.STRIDES, ai.OCTAVE, torch.float32)):
        assert torch.equal(a, b)


def test_float64_assignment_agrees_with_the_fixture(gold):
    """the restated assignment gives the reference's gt_inds, evaluated in float32 (the reference's own comparisons) and in
    float64 (no decision of these inputs sits on a rounding edge); and the conditions the generator settled its seed on"""
    gt_bboxes, _ = ai.gts(int(gold['seed_assign']))
    for dtype in (torch.float32, torch.float64):
        inds, info = R.assign(gt_bboxes, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK, dtype=dtype, details=True)
        for b in range(2):
            assert np.array_equal(inds[b].numpy(), gold[f'assign_gt_inds{b}']), (b, dtype)
            got = info[b]['max_overlaps'].numpy()
            assert np.allclose(got, gold[f'assign_max_overlaps{b}'], rtol=4 * EPS32, atol=0), (b, dtype)
    _, info = R.assign(gt_bboxes, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK, dtype=torch.float32, details=True)
    assert sum(int(((d['iou'] >= d['thr'][None]) & ~(d['side'] > 0.01)).sum()) for d in info) > 0     # the centre test bites
    assert sum(int((torch.isfinite(d['claimed']).sum(1) >= 2).sum()) for d in info) > 0               # a contested anchor
    assert all(float(d['gaps'].min()) > 0 for d in info)
    assert info[0]['cand'].shape[0] == 9 + 9 + 9 + 6 + 2                                              # levels below topk


@pytest.mark.parametrize('C', [4, 1])
def test_float64_loss_agrees_with_the_fixture(gold, C):
    """the fixture is ONE fp32 evaluation of the same sums, by torch on the CPU: a few dozen positive terms and up to 768 x C
    focal terms per level, each a handful of roundings, summed pairwise.  64 eps of the value covers that (the same order as
    the rtol of 1e-5 the host mirror is held to above); the float64 gradients agree with the reference's autograd gradients
    to 1e-4 of the largest gradient of their tensor"""
    tag = f'loss_c{C}'
    seed = int(gold[f'seed_{tag}'])
    cls, raw, ctr = ai.head_outputs(seed, C)
    gt_bboxes, gt_labels = ai.gts(seed, num_classes=C)
    inds = R.assign(gt_bboxes, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK, dtype=torch.float32)
    ref = R.loss(cls, raw, ctr, ai.SCALES, inds, gt_bboxes, gt_labels, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.MEANS, ai.STDS,
                 weights=(1.0, 2.0, 1.0))
    assert ref['n_pos'] > 5
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_centerness')):
        want = gold[f'{tag}_{k}'].astype(np.float64)
        assert (np.abs(ref['losses'][i].numpy() - want) <= 64 * EPS32 * np.abs(want)).all(), (k, ref['losses'][i], want)
    if C == 4:
        for l in range(L):
            for name, key in (('dcls', 'dcls'), ('dreg', 'draw'), ('dctr', 'dctr')):
                g = gold[f'{tag}_{name}{l}'].astype(np.float64)
                assert np.abs(ref[key][l].numpy() - g).max() <= 1e-4 * max(np.abs(g).max(), 1e-12), (name, l)
        g = gold[f'{tag}_dscale'].astype(np.float64)
        assert np.abs(ref['dscale'].numpy() - g).max() <= 1e-4 * np.abs(g).max()


def test_float64_candidates_agree_with_the_host_mirror(gold):
    """the restated decode against the head's own torch chain (clip to the image, rescale)"""
    from brcnn.core import delta2bbox
    seed = int(gold['seed_bboxes_c4'])
    head = build(4)
    cls, raw, ctr = ai.head_outputs(seed, 4)
    metas = ai.metas()
    ref = R.candidates(cls, raw, ctr, ai.SCALES, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.MEANS, ai.STDS,
                       [m['img_shape'] for m in metas])
    for l, an in enumerate(grid(head)):
        for b in range(2):
            d = (raw[l][b] * ai.SCALES[l]).permute(1, 2, 0).reshape(-1, 4)
            want = delta2bbox(an, d, ai.MEANS, ai.STDS, max_shape=tuple(metas[b]['img_shape'][:2]))
            assert np.allclose(ref[l][3][b].numpy(), want.numpy(), rtol=1e-5, atol=1e-4), (l, b)
