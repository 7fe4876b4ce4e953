"""CPU tests (-m "not gpu") of the GFL baseline: the recipe builds and equals the reference's, its parameters are the
reference's, the refused settings raise with their names, the two loss modules give hand-computed values, the torch host
mirrors of GFLHead.get_targets / loss / get_bboxes reproduce what the reference computed (tests/golden/g30_gfl.npz, made by
tests/golden/make_golden_gfl.py), and the float64 restatement (tests/gfl_ref64.py) is pinned to the fixture before the GPU
tests lean on it."""
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
from tests import gfl_inputs as gi
from tests import gfl_ref64 as R

G = os.path.join(os.path.dirname(__file__), 'golden', 'g30_gfl.npz')
REF_CONFIG = '/root/reference/configs/gfl/gfl_r50_fpn_1x_coco.py'
EPS32 = float(np.finfo(np.float32).eps)
L = len(gi.SIZES)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(gi.CONFIG).model)


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(gi.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, gi.SCALES):
            s.scale.fill_(v)
    return head


def test_config_builds_the_baseline(model):
    from brcnn.core import ATSSAssigner
    from brcnn.dense_heads import ATSSHead, GFLHead, GNTowerHead
    from brcnn.detectors import GFL, SingleStageDetector
    from brcnn.losses import DistributionFocalLoss, GIoULoss, QualityFocalLoss
    from brcnn.necks import FPN
    from brcnn.registry import DETECTORS, HEADS, LOSSES
    assert HEADS.get('GFLHead') is GFLHead and DETECTORS.get('GFL') is GFL
    assert LOSSES.get('QualityFocalLoss') is QualityFocalLoss and LOSSES.get('DistributionFocalLoss') is DistributionFocalLoss
    assert type(model) is GFL and isinstance(model, SingleStageDetector)
    assert type(model.bbox_head) is GFLHead and type(model.neck) is FPN
    h = model.bbox_head
    assert isinstance(h, GNTowerHead) and not isinstance(h, ATSSHead)
    assert h.cls_out_channels == 4 and h.strides == gi.STRIDES and h.stacked_convs == 4 and h.num_anchors == 1 and h.reg_max == 16
    assert type(h.assigner) is ATSSAssigner and h.assigner.topk == 9
    assert type(h.loss_cls) is QualityFocalLoss and h.loss_cls.beta == 2.0 and h.loss_cls.loss_weight == 1.0
    assert type(h.loss_dfl) is DistributionFocalLoss and h.loss_dfl.loss_weight == 0.25
    assert type(h.loss_bbox) is GIoULoss and h.loss_bbox.loss_weight == 2.0
    assert h.integral.project.tolist() == list(range(17))
    assert h.test_cfg.nms_pre == 1000 and h.test_cfg.max_per_img == 100 and h.test_cfg.nms.iou_threshold == 0.6
    assert not model.with_rpn and not model.with_roi_head and not h.supports_tta
    h._check_limits(h.test_cfg, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])       # the recipe's sizes (800 x 1344)
    assert 'configs/gfl' in open(os.path.join(gi.ROOT, 'tools', 'bench_recipes.py')).read()


@pytest.mark.skipif(not os.path.isfile(REF_CONFIG), reason='reference tree absent')
def test_shipped_config_equals_the_reference_config():
    """the reference recipe loads UNCHANGED through this repo's loader and equals the shipped rewrite key for key"""
    r = Config.fromfile(REF_CONFIG).to_dict()
    assert 'model' in r and r['model']['type'] == 'GFL'
    assert Config.fromfile(gi.CONFIG).to_dict() == r


def test_parameter_names_and_shapes_are_the_references(model, gold):
    sd = model.state_dict()
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want
    assert list(sd) == [str(k) for k in gold['state_keys']]
    fresh = build_detector(Config.fromfile(gi.CONFIG).model)
    res = fresh.load_state_dict({str(k): torch.zeros(json.loads(str(s))) for k, s in zip(gold['state_keys'], gold['state_shapes'])})
    assert not res.missing_keys and not res.unexpected_keys
    h = build_head(ConfigDict(gi.head_cfg(num_classes=3, in_channels=16, feat_channels=32, stacked_convs=1, reg_max=7)))
    assert [k for k in h.state_dict()] == [
        'cls_convs.0.conv.weight', 'cls_convs.0.gn.weight', 'cls_convs.0.gn.bias',
        'reg_convs.0.conv.weight', 'reg_convs.0.gn.weight', 'reg_convs.0.gn.bias',
        'gfl_cls.weight', 'gfl_cls.bias', 'gfl_reg.weight', 'gfl_reg.bias',
        'scales.0.scale', 'scales.1.scale', 'scales.2.scale', 'scales.3.scale', 'scales.4.scale', 'integral.project']
    assert h.gfl_cls.weight.shape == (3, 32, 3, 3) and h.gfl_reg.weight.shape == (32, 32, 3, 3)
    assert h.integral.project.tolist() == list(range(8)) and h.scales[0].scale.shape == ()
    # Normal(0, 0.01) convs, zero biases but gfl_cls's, which starts at the prior 0.01
    assert torch.allclose(h.gfl_cls.bias, torch.full((3,), -float(np.log(99.0))))
    assert float(h.gfl_reg.bias.detach().abs().max()) == 0 and 0.005 < float(h.cls_convs[0].conv.weight.detach().std()) < 0.02


def _ag(**kw):
    return dict(dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=2, scales_per_octave=1, strides=gi.STRIDES), **kw)


def _tc(**kw):
    return dict(dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False), **kw)


QFL = dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0)
REFUSED = [
    (dict(anchor_generator=_ag(ratios=[0.5, 1.0])), NotImplementedError, 'anchors per cell'),
    (dict(anchor_generator=_ag(scales_per_octave=2)), NotImplementedError, 'scales_per_octave'),
    (dict(anchor_generator=_ag(strides=[(8, 16), (16, 16), (32, 32), (64, 64), (128, 128)])), NotImplementedError, 'square strides'),
    (dict(norm_cfg=None), NotImplementedError, 'norm_cfg'),
    (dict(norm_cfg=dict(type='BN', requires_grad=True)), NotImplementedError, 'norm_cfg'),
    (dict(loss_cls=dict(type='FocalLoss', use_sigmoid=True, loss_weight=1.0)), NotImplementedError, 'loss_cls'),
    (dict(loss_cls=dict(QFL, use_sigmoid=False)), NotImplementedError, 'loss_cls'),
    (dict(loss_cls=dict(QFL, beta=0.5)), NotImplementedError, 'beta'),
    (dict(loss_bbox=dict(type='L1Loss', loss_weight=1.0)), NotImplementedError, 'loss_bbox'),
    (dict(loss_bbox=dict(type='IoULoss', loss_weight=1.0)), NotImplementedError, 'loss_bbox'),
    (dict(loss_dfl=dict(type='CrossEntropyLoss', loss_weight=0.25)), NotImplementedError, 'loss_dfl'),
    (dict(loss_cls=dict(QFL, reduction='sum')), NotImplementedError, 'reduction'),
    (dict(loss_bbox=dict(type='GIoULoss', reduction='sum')), NotImplementedError, 'reduction'),
    (dict(loss_dfl=dict(type='DistributionFocalLoss', reduction='none')), NotImplementedError, 'reduction'),
    (dict(reg_max=0), ValueError, 'reg_max'),
    (dict(reg_max=17), ValueError, 'reg_max'),
    (dict(train_cfg=_tc(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4))), NotImplementedError, 'assigner'),
    (dict(train_cfg=_tc(pos_weight=2.0)), NotImplementedError, 'pos_weight'),
    (dict(train_cfg=_tc(allowed_border=0)), NotImplementedError, 'allowed_border'),
    (dict(test_cfg=dict(gi.TEST_CFG, nms=dict(type='soft_nms', iou_threshold=0.5))), NotImplementedError, 'soft'),
    (dict(test_cfg=dict(gi.TEST_CFG, nms=dict(type='nms', iou_threshold=0.5, class_agnostic=True))), NotImplementedError,
     'class_agnostic'),
]


@pytest.mark.parametrize('over,exc,name', REFUSED, ids=[f'{i}-{n}' for i, (_, _, n) in enumerate(REFUSED)])
def test_refused_settings_raise_with_their_name(over, exc, name):
    with pytest.raises(exc, match=name):
        build_head(ConfigDict(gi.head_cfg(**over)))


def test_refused_calls_raise_with_their_name(model):
    head = build()
    cls, raw = gi.head_outputs(3)
    with pytest.raises(NotImplementedError, match='with_nms=False'):
        head.get_bboxes(cls, gi.scaled(raw, gi.SCALES), gi.metas(), with_nms=False)
    with pytest.raises(NotImplementedError, match='gt_bboxes_ignore'):
        head.forward_train_nhwc(None, gi.metas(), None, None, gt_bboxes_ignore=[torch.zeros(0, 4)] * 2)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(gi.TEST_CFG, nms_pre=5000), gi.SIZES)
    with pytest.raises(ValueError, match='nms_pre'):
        head._check_limits(ConfigDict(gi.TEST_CFG, nms_pre=-1), gi.SIZES)
    imgs = [torch.zeros(1, 3, gi.H, gi.W), torch.zeros(1, 3, gi.H, gi.W)]
    metas = [gi.metas(1), [dict(gi.metas(1)[0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.forward_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        head.aug_test(None, metas)


# ------------------------------------------------------------------------------------------- the two loss modules by hand
def test_quality_focal_loss_by_hand():
    from brcnn.losses import QualityFocalLoss
    sp = lambda x: math.log1p(math.exp(x))      # noqa: E731  BCE(x, 0)
    sg = lambda x: 1 / (1 + math.exp(-x))       # noqa: E731
    pred = torch.tensor([[0.5, -1.0], [2.0, 0.0], [-0.3, 0.7]], dtype=torch.float64)
    label, score = torch.tensor([1, 2, 0]), torch.tensor([0.8, 0.0, 0.25], dtype=torch.float64)
    for beta in (2.0, 1.5):
        bg = lambda x: sp(x) * sg(x) ** beta                                        # noqa: E731
        fg = lambda x, q: ((1 - q) * x + sp(-x)) * abs(q - sg(x)) ** beta           # noqa: E731  BCE(x, q) = (1-q)x + softplus(-x)
        rows = [bg(0.5) + fg(-1.0, 0.8), bg(2.0) + bg(0.0), fg(-0.3, 0.25) + bg(0.7)]      # row 1: background (label 2 = C)
        m = QualityFocalLoss(beta=beta, loss_weight=0.5)
        got = m(pred, (label, score), reduction_override='none')
        assert np.allclose(got.numpy(), [0.5 * r for r in rows], rtol=1e-12, atol=0)
        w = torch.tensor([1.0, 0.0, 2.0], dtype=torch.float64)
        assert math.isclose(float(m(pred, (label, score), weight=w, avg_factor=3.0)), 0.5 * (rows[0] + 2 * rows[2]) / 3.0,
                            rel_tol=1e-12)
        assert math.isclose(float(m(pred, (label, score))), 0.5 * sum(rows) / 3, rel_tol=1e-12)
    with pytest.raises(AssertionError):
        QualityFocalLoss(use_sigmoid=False)


def test_distribution_focal_loss_by_hand():
    from brcnn.losses import DistributionFocalLoss
    pred = torch.tensor([[0.0, 1.0, 2.0, -1.0], [3.0, 0.0, 0.0, 0.0], [0.2, 0.2, 0.2, 0.2]], dtype=torch.float64)
    label = torch.tensor([1.25, 0.0, 2.9], dtype=torch.float64)

    def ce(row, i):
        return math.log(sum(math.exp(v) for v in row)) - row[i]
    p = pred.tolist()
    rows = [ce(p[0], 1) * 0.75 + ce(p[0], 2) * 0.25,
            ce(p[1], 0) * 1.0 + ce(p[1], 1) * 0.0,             # an integer target: the right bin has weight 0
            ce(p[2], 2) * (3 - 2.9) + ce(p[2], 3) * (2.9 - 2)]
    m = DistributionFocalLoss(loss_weight=0.25)
    assert np.allclose(m(pred, label, reduction_override='none').numpy(), [0.25 * r for r in rows], rtol=1e-12, atol=0)
    w = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)
    assert math.isclose(float(m(pred, label, weight=w, avg_factor=4.0)),
                        0.25 * (0.5 * rows[0] + rows[1] + 2 * rows[2]) / 4.0, rel_tol=1e-12)
    assert math.isclose(rows[2], math.log(4.0), rel_tol=1e-12)      # a flat distribution: log(n + 1) whatever the target


# ------------------------------------------------------------------------------------------- host mirror vs the fixture
def test_get_targets_host_mirror_is_exact(gold):
    head = build(4, True)
    gt_bboxes, gt_labels = gi.gts(int(gold['seed_targets']))
    anchor_list, valid_flag_list = head.get_anchors(gi.SIZES, gi.metas(), device='cpu')
    out = head.get_targets(anchor_list, valid_flag_list, gt_bboxes, gi.metas(), gt_labels_list=gt_labels, label_channels=4)
    _, labels, weights, targets, _, num_pos, num_neg = out
    for l in range(L):
        assert np.array_equal(labels[l].numpy(), gold[f'targets_labels{l}']), l
        assert np.array_equal(weights[l].numpy(), gold[f'targets_weights{l}']), l
        assert np.array_equal(targets[l].numpy(), gold[f'targets_box{l}']), l           # the ground-truth boxes themselves
    assert [num_pos, num_neg] == gold['targets_num'].tolist()
    assert sum(bool((labels[l] < 4).any()) for l in range(L)) >= 3


@pytest.mark.parametrize('C', [4, 1])
def test_loss_host_mirror_reproduces_the_reference(gold, C):
    tag = f'loss_c{C}'
    seed = int(gold[f'seed_{tag}'])
    head = build(C, True)
    cls, raw = gi.head_outputs(seed, C, grad=True)
    scales = [torch.tensor(v, requires_grad=True) for v in gi.SCALES]
    gt_bboxes, gt_labels = gi.gts(seed, num_classes=C)
    losses = head.loss(cls, gi.scaled(raw, scales), gt_bboxes, gt_labels, gi.metas())
    assert sorted(losses) == ['loss_bbox', 'loss_cls', 'loss_dfl']
    for k, v in losses.items():
        got = torch.stack([torch.as_tensor(x) for x in v]).detach().numpy()
        assert len(v) == L and np.allclose(got, gold[f'{tag}_{k}'], rtol=1e-5, atol=1e-7), (k, got, gold[f'{tag}_{k}'])
    sum(sum(v) for v in losses.values()).backward()
    assert all(torch.isfinite(t.grad).all() for t in cls + raw)
    if C == 4:
        for l in range(L):
            for name, t in (('dcls', cls), ('dreg', raw)):
                assert np.allclose(t[l].grad.numpy(), gold[f'{tag}_{name}{l}'], rtol=1e-4, atol=1e-8), (name, l)
        assert np.allclose(torch.stack([s.grad for s in scales]).numpy(), gold[f'{tag}_dscale'], rtol=1e-4, atol=1e-8)


def test_loss_host_mirror_without_ground_truth():
    head = build(4, True)
    cls, raw = gi.head_outputs(5, grad=True)
    empty = [torch.zeros(0, 4), torch.zeros(0, 4)], [torch.zeros(0, dtype=torch.long)] * 2
    losses = head.loss(cls, gi.scaled(raw, gi.SCALES), *empty, gi.metas())
    assert all(x.item() == 0 for x in losses['loss_bbox']) and all(x.item() == 0 for x in losses['loss_dfl'])
    assert sum(losses['loss_cls']).item() > 0


CASES = [(4, 'plain'), (4, 'rescale'), (4, 'empty'), (1, 'plain'), (1, 'rescale')]


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_host_mirror_reproduces_the_reference(gold, C, name):
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C)
    cls, raw = gi.head_outputs(seed, C, empty=(name == 'empty'))
    res = head.get_bboxes(cls, gi.scaled(raw, gi.SCALES), gi.metas(), rescale=(name != 'plain'), batched_nms=orc.batched_nms)
    for b, (det, lab) in enumerate(res):
        want_d, want_l = gold[f'bboxes_c{C}_{name}_det{b}'], gold[f'bboxes_c{C}_{name}_lab{b}']
        assert lab.tolist() == want_l.tolist(), (C, name, b)
        assert det.shape == want_d.shape and np.allclose(det.numpy(), want_d, rtol=0, atol=1e-5), (C, name, b)
    if name == 'empty':
        assert len(res[1][0]) == 0 and len(res[0][0]) > 0


def test_forward_host_mirror_shapes():
    head = build(3, reg_max=7)
    g = torch.Generator().manual_seed(0)
    feats = [torch.randn(2, 64, h, w, generator=g) for h, w in gi.SIZES]
    cls, reg = head(feats)
    assert [tuple(c.shape) for c in cls] == [(2, 3, h, w) for h, w in gi.SIZES]
    assert [tuple(r.shape) for r in reg] == [(2, 32, h, w) for h, w in gi.SIZES] and reg[0].dtype == torch.float32


# ------------------------------------------------------------------------------------------- float64 restatement pinned
@pytest.mark.parametrize('C', [4, 1])
def test_float64_loss_agrees_with_the_fixture(gold, C):
    """the fixture is ONE fp32 evaluation of the same sums, by torch on the CPU: a few dozen positive terms and up to 768 x C
    class terms per level, each a handful of roundings, summed pairwise.  64 eps of the value covers the class and box sums
    (the same order as the rtol of 1e-5 the host mirror is held to above); the DFL terms are differences of logits of size
    ~10 and a log-sum-exp, so their sum is held to 64 eps of 10 x the number of positive sides instead of its own value.  The
    float64 gradients agree with the reference's autograd gradients to 1e-4 of the largest gradient of their tensor"""
    tag = f'loss_c{C}'
    seed = int(gold[f'seed_{tag}'])
    cls, raw = gi.head_outputs(seed, C)
    gt_bboxes, gt_labels = gi.gts(seed, num_classes=C)
    inds = RA.assign(gt_bboxes, gi.SIZES, gi.STRIDES, gi.OCTAVE, gi.TOPK, dtype=torch.float32)
    ref = R.loss(cls, raw, gi.SCALES, inds, gt_bboxes, gt_labels, gi.SIZES, gi.STRIDES, gi.OCTAVE, weights=(1.0, 2.0, 0.25),
                 bounds=False)
    assert ref['n_pos'] > 5
    frac = ref['side'] - ref['side'].round()
    assert float(frac.abs().min()) > 1e-4                                       # the generator's condition on the bins
    for i, k in enumerate(('loss_cls', 'loss_bbox', 'loss_dfl')):
        want = gold[f'{tag}_{k}'].astype(np.float64)
        tol = 64 * EPS32 * np.abs(want) + (64 * EPS32 * 0.25 * 10 * ref['n_pos'] / max(ref['norm2'][1], 1.0) if i == 2 else 0)
        assert (np.abs(ref['losses'][i].numpy() - want) <= tol).all(), (k, ref['losses'][i], want)
    if C == 4:
        for l in range(L):
            for name, key in (('dcls', 'dcls'), ('dreg', 'draw')):
                g = gold[f'{tag}_{name}{l}'].astype(np.float64)
                assert np.abs(ref[key][l].numpy() - g).max() <= 1e-4 * max(np.abs(g).max(), 1e-12), (name, l)
        g = gold[f'{tag}_dscale'].astype(np.float64)
        assert np.abs(ref['dscale'].numpy() - g).max() <= 1e-4 * np.abs(g).max()


def test_float64_candidates_agree_with_the_host_mirror(gold):
    """the restated decode against the head's own torch chain (integral, clip to the image, rescale)"""
    from brcnn.dense_heads import distance2bbox
    seed = int(gold['seed_bboxes_c4'])
    head = build(4)
    cls, raw = gi.head_outputs(seed, 4)
    metas = gi.metas()
    ref = R.candidates(cls, raw, gi.SCALES, gi.SIZES, gi.STRIDES, [m['img_shape'] for m in metas])
    for l, an in enumerate(head.anchor_generator.grid_anchors(gi.SIZES, 'cpu')):
        for b in range(2):
            h, w = metas[b]['img_shape'][:2]
            d = head.integral((raw[l][b] * gi.SCALES[l]).permute(1, 2, 0)) * gi.STRIDES[l]
            want = distance2bbox(head.anchor_center(an), d)
            want = torch.stack([want[:, 0].clamp(0, w), want[:, 1].clamp(0, h), want[:, 2].clamp(0, w), want[:, 3].clamp(0, h)], -1)
            assert np.allclose(ref[l][2][b].numpy(), want.numpy(), rtol=1e-5, atol=1e-3), (l, b)
            assert float(ref[l][3][b].max()) < 0.1


def test_float64_error_records_are_finite():
    """the first-order error records the GPU test builds its bounds from exist for every positive and are small"""
    seed = 44
    cls, raw = gi.head_outputs(seed, 4)
    gt_bboxes, gt_labels = gi.gts(seed)
    inds = RA.assign(gt_bboxes, gi.SIZES, gi.STRIDES, gi.OCTAVE, gi.TOPK, dtype=torch.float32)
    ref = R.loss(cls, raw, gi.SCALES, inds, gt_bboxes, gt_labels, gi.SIZES, gi.STRIDES, gi.OCTAVE)
    P = ref['n_pos']
    assert P > 5 and ref['dx_box_err'].shape == (P, 4, 17) and ref['dx_dfl_err'].shape == (P, 4, 17)
    for k in ('box_value_err', 'dfl_value_err', 'quality_err', 'hit_value_err', 'dhit_err', 'dx_box_err', 'dx_dfl_err'):
        assert torch.isfinite(ref[k]).all() and float(ref[k].max()) < 1e-3, k
