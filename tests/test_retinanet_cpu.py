"""CPU tests (-m "not gpu") of the RetinaNet baseline: the recipe builds and equals the reference's, its parameters are the
reference's, the refused settings raise with their names, the torch host mirror of RetinaHead.get_bboxes / loss reproduces
what the reference computed (tests/golden/g27_retinanet.npz, made by tests/golden/make_golden_retinanet.py), and the float64
reference of the dense loss (tests/dense_loss_ref64.py) is pinned to the fixture before the GPU tests lean on it."""
import json
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, build_head
from brcnn.config import ConfigDict
from oracle import orc
from tests import dense_loss_ref64 as R
from tests import retinanet_inputs as ri

G = os.path.join(os.path.dirname(__file__), 'golden', 'g27_retinanet.npz')
REF_CONFIG = '/root/reference/configs/retinanet/retinanet_r50_fpn_1x_coco.py'
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(ri.CONFIG).model)


def test_config_builds_the_baseline(model):
    from brcnn.dense_heads import RetinaHead
    from brcnn.detectors import RetinaNet, SingleStageDetector
    from brcnn.necks import FPN
    assert type(model) is RetinaNet and isinstance(model, SingleStageDetector)
    assert type(model.bbox_head) is RetinaHead and type(model.neck) is FPN
    h = model.bbox_head
    assert h.num_anchors == 9 and h.cls_out_channels == 4 and [s[0] for s in h.anchor_generator.strides] == ri.STRIDES
    a = h.assigner
    assert (a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou, a.match_low_quality) == (0.5, 0.4, 0, True)
    assert type(h.sampler).__name__ == 'PseudoSampler' and not h.sampling
    assert (h.loss_cls.gamma, h.loss_cls.alpha) == (2.0, 0.25) and type(h.loss_bbox).__name__ == 'L1Loss'
    assert h.test_cfg.nms_pre == 1000 and h.test_cfg.max_per_img == 100 and h.test_cfg.score_thr == 0.05
    assert not model.with_rpn and not model.with_roi_head
    # the device path accepts the recipe's sizes (800 x 1344)
    h._check_limits(h.test_cfg, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])
    cfg = Config.fromfile(ri.CONFIG)
    assert cfg.optimizer.lr == 0.005 and cfg.data.samples_per_gpu == 4


@pytest.mark.skipif(not os.path.isfile(REF_CONFIG), reason='reference tree absent')
def test_shipped_config_equals_the_reference_config():
    """the reference recipe loads UNCHANGED through this repo's loader and equals the shipped rewrite key for key (the
    comparison of tests/test_host_cpu.py::test_shipped_configs_equal_reference_configs)"""
    r = Config.fromfile(REF_CONFIG).to_dict()
    assert 'model' in r and r['model']['type'] == 'RetinaNet'
    assert Config.fromfile(ri.CONFIG).to_dict() == r


def test_parameter_names_and_shapes_are_the_references(model, gold):
    sd = model.state_dict()
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want
    h = build_head(ConfigDict(ri.head_cfg(num_classes=3, in_channels=16, feat_channels=8, stacked_convs=2)))
    assert [k for k in h.state_dict()] == [
        'cls_convs.0.conv.weight', 'cls_convs.0.conv.bias', 'cls_convs.1.conv.weight', 'cls_convs.1.conv.bias',
        'reg_convs.0.conv.weight', 'reg_convs.0.conv.bias', 'reg_convs.1.conv.weight', 'reg_convs.1.conv.bias',
        'retina_cls.weight', 'retina_cls.bias', 'retina_reg.weight', 'retina_reg.bias']
    assert h.retina_cls.weight.shape == (27, 8, 3, 3) and h.retina_reg.weight.shape == (36, 8, 3, 3)
    # Normal(0, 0.01) convs, zero biases but retina_cls's, which starts at the prior 0.01
    assert torch.allclose(h.retina_cls.bias, torch.full((27,), -float(np.log(99.0))))
    assert float(h.retina_reg.bias.detach().abs().max()) == 0 and 0.005 < float(h.cls_convs[1].conv.weight.detach().std()) < 0.02


REFUSED = [
    (dict(norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)), 'norm_cfg'),
    (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)), 'use_sigmoid=False'),
    (dict(reg_decoded_bbox=True), 'reg_decoded_bbox=True'),
    (dict(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)), 'loss_cls'),
    (dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)), 'loss_bbox'),
    (dict(train_cfg=dict(ri.head_cfg()['train_cfg'], sampler=dict(type='RandomSampler', num=256, pos_fraction=0.5))),
     'sampler'),
    (dict(test_cfg=dict(ri.TEST_CFG, nms=dict(type='soft_nms', iou_threshold=0.5))), 'soft'),
    (dict(test_cfg=dict(ri.TEST_CFG, nms=dict(type='nms', iou_threshold=0.5, class_agnostic=True))), 'class_agnostic'),
]


@pytest.mark.parametrize('over,name', REFUSED, ids=[n for _, n in REFUSED])
def test_refused_settings_raise_with_their_name(over, name):
    with pytest.raises(NotImplementedError, match=name):
        build_head(ConfigDict(ri.head_cfg(**over)))


def test_refused_calls_raise_with_their_name(model):
    head = build_head(ConfigDict(ri.head_cfg()))
    cls, reg = ri.head_outputs(3)
    with pytest.raises(NotImplementedError, match='with_nms=False'):
        head.get_bboxes(cls, reg, ri.metas(), with_nms=False)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(ri.TEST_CFG, nms_pre=5000), ri.SIZES)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(ri.TEST_CFG, nms_pre=-1), ri.SIZES)
    imgs = [torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 64, 96)]
    metas = [ri.metas(1), [dict(ri.metas(1)[0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.forward_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        head.aug_test(None, metas)


# ------------------------------------------------------------------------------------------- host mirror vs the fixture
CASES = [(c, name) for c in ri.CLASS_COUNTS for name in ('plain', 'rescale')] + [(4, 'empty')]


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_host_mirror_reproduces_the_reference(gold, C, name):
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build_head(ConfigDict(ri.head_cfg(C))).eval()
    cls, reg = ri.head_outputs(seed, C, empty=(name == 'empty'))
    res = head.get_bboxes(cls, reg, ri.metas(), rescale=(name != 'plain'), batched_nms=orc.batched_nms)
    for b, (det, lab) in enumerate(res):
        want_d, want_l = gold[f'bboxes_c{C}_{name}_det{b}'], gold[f'bboxes_c{C}_{name}_lab{b}']
        assert lab.tolist() == want_l.tolist(), (C, name, b)
        assert det.shape == want_d.shape and np.allclose(det.numpy(), want_d, rtol=0, atol=1e-5), (C, name, b)
    if name == 'empty':
        assert len(res[1][0]) == 0 and len(res[0][0]) > 0


@pytest.mark.parametrize('tag,C,loss_bbox', [('loss_l1', 4, dict(type='L1Loss', loss_weight=1.0)),
                                             ('loss_sl1', 1, dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0))])
def test_loss_host_mirror_reproduces_the_reference(gold, tag, C, loss_bbox):
    seed = int(gold[f'seed_{tag}'])
    head = build_head(ConfigDict(ri.head_cfg(C, loss_bbox=loss_bbox))).train()
    cls, reg = ri.head_outputs(seed, C, grad=True)
    gt_bboxes, gt_labels = ri.gts(seed, num_classes=C)
    losses = head.loss(cls, reg, gt_bboxes, gt_labels, ri.metas())
    assert sorted(losses) == ['loss_bbox', 'loss_cls'] and len(losses['loss_cls']) == len(ri.SIZES)
    for k in ('loss_cls', 'loss_bbox'):
        got = torch.stack(losses[k]).detach().numpy()
        assert np.allclose(got, gold[f'{tag}_{k}'], rtol=1e-5, atol=1e-7), (k, got, gold[f'{tag}_{k}'])
    sum(losses['loss_cls'] + losses['loss_bbox']).backward()
    assert all(torch.isfinite(t.grad).all() for t in cls + reg)
    if tag == 'loss_l1':
        for l, (c, r) in enumerate(zip(cls, reg)):
            assert np.allclose(c.grad.numpy(), gold[f'{tag}_dcls{l}'], rtol=1e-4, atol=1e-8), l
            assert np.allclose(r.grad.numpy(), gold[f'{tag}_dreg{l}'], rtol=1e-4, atol=1e-8), l


# ------------------------------------------------------------------------------------------- float64 reference pinned
def ref64_case(seed, C, beta=0.0, pos_weight=-1.0):
    """the float64 reference on the seeded head-level inputs, with the assignment of the host assigner"""
    head = build_head(ConfigDict(ri.head_cfg(C)))
    cls, reg = ri.head_outputs(seed, C)
    gt_bboxes, gt_labels = ri.gts(seed, num_classes=C)
    anchors = torch.cat(head.anchor_generator.grid_anchors(ri.SIZES, 'cpu'))
    gt_inds = torch.stack([head.assigner.assign(anchors, g, None, None).gt_inds for g in gt_bboxes])
    offs = [0]
    for g in gt_bboxes:
        offs.append(offs[-1] + len(g))
    x, p, level_sizes = R.flatten_outputs([c.numpy() for c in cls], [r.numpy() for r in reg], C)
    ref = R.dense_loss(x, p, level_sizes, anchors.numpy(), gt_inds.numpy(), torch.cat(gt_bboxes).numpy(),
                       torch.cat(gt_labels).numpy(), offs, beta=beta, pos_weight=pos_weight)
    return ref, cls, reg


@pytest.mark.parametrize('tag,C,beta', [('loss_l1', 4, 0.0), ('loss_sl1', 1, 1.0 / 9.0)])
def test_float64_reference_agrees_with_the_fixture(gold, tag, C, beta):
    """the fixture is ONE fp32 evaluation of the same per-level sums: each sits within the fp32 bound of the float64
    value (summation in any order + the evaluation error of the terms), plus the rounding of the stored number; the
    float64 gradients agree with the reference's autograd gradients to fp32 round-off of the latter"""
    ref, cls, reg = ref64_case(int(gold[f'seed_{tag}']), C, beta)
    assert ref['num_total_pos'] > 2 and (ref['n_pos'] > 0).all()
    for k, t in (('loss_cls', 'tol_cls'), ('loss_bbox', 'tol_bbox')):
        want = gold[f'{tag}_{k}'].astype(np.float64)
        assert (np.abs(ref[k] - want) <= ref[t] + 4 * EPS32 * np.abs(want)).all(), (k, ref[k], want, ref[t])
    assert ref['loss_bbox'][0] > 0
    if tag == 'loss_l1':
        dcls, dreg = R.unflatten(ref['dx'], ref['dpred'], ri.SIZES, ri.A)
        ecls, ereg = R.unflatten(ref['dx_err'], ref['dpred_err'], ri.SIZES, ri.A)
        _, sure = R.unflatten(ref['dx'], ref['dpred_sure'].astype(np.float64), ri.SIZES, ri.A)
        # The reference's host form is BCE-with-logits x alpha_t x miss^gamma (focal_loss.py:12-57), differentiated by
        # autograd.  Its BCE value is max(x, 0) - x t + log1p(exp(-|x|)) in fp32: for a confident logit two terms of size
        # |x| cancel, an ABSOLUTE error of eps (|x| + 2), which reaches the gradient through d(alpha_t miss^gamma)/dx =
        # alpha_t gamma miss^gamma (1 - miss).  That share belongs to the fixture, not to the float64 value.
        x, _, _ = R.flatten_outputs([c.numpy() for c in cls], [r.numpy() for r in reg], C)
        p = 1.0 / (1.0 + np.exp(-x))
        miss, alpha_t = np.where(ref['hit'], 1.0 - p, p), np.where(ref['hit'], 0.25, 0.75)
        bce_share = ref['weight'][..., None] / ref['num_total_pos'] * alpha_t * 2.0 * miss ** 2 * (1.0 - miss) * \
            EPS32 * (np.abs(x) + 2.0)
        fcls, _ = R.unflatten(bce_share, ref['dpred'], ri.SIZES, ri.A)
        for l in range(len(ri.SIZES)):
            gc, gr = gold[f'{tag}_dcls{l}'].astype(np.float64), gold[f'{tag}_dreg{l}'].astype(np.float64)
            # (its sigmoid carries the same cancellation in 1 - p as the kernel's: one more share of the element's bound)
            assert (np.abs(dcls[l] - gc) <= 2 * ecls[l] + fcls[l] + 4 * EPS32 * np.abs(gc) + 1e-30).all(), l
            ok = sure[l] > 0                # (where the sign of pred - target is determined in fp32)
            assert (np.abs(dreg[l] - gr)[ok] <= (ereg[l] + 4 * EPS32 * np.abs(gr))[ok] + 1e-30).all(), l
