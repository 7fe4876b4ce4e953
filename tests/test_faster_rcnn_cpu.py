"""CPU tests (-m "not gpu") of the Faster R-CNN baseline: the recipe builds, its parameters are the reference's, the torch
host path of RPNHead.loss / BBoxHead.loss reproduces what the reference computed (tests/golden/g25_faster_rcnn.npz, made
by tests/golden/make_golden_faster_rcnn.py), the refused configurations raise, and the float64 reference of the sampled
RPN loss (tests/rpn_sampled_ref64.py) is pinned to the fixture before the GPU tests lean on it."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brcnn  # noqa: F401
from brcnn import Config, build_detector, build_head, core
from brcnn.config import ConfigDict
from oracle import orc
from tests import faster_rcnn_inputs as fi
from tests import rpn_sampled_ref64 as R
from tests import util

G = os.path.join(os.path.dirname(__file__), 'golden', 'g25_faster_rcnn.npz')
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(fi.CONFIG).model)


def test_config_builds_the_baseline(model):
    from brcnn.dense_heads import RPNHead
    from brcnn.necks import FPN
    from brcnn.roi_heads import Shared2FCBBoxHead, StandardRoIHead
    assert type(model.rpn_head) is RPNHead and type(model.roi_head) is StandardRoIHead
    assert type(model.neck) is FPN and type(model.roi_head.bbox_head) is Shared2FCBBoxHead
    assert model.rpn_head.num_anchors == 3 and [s[0] for s in model.rpn_head.anchor_generator.strides] == [4, 8, 16, 32, 64]
    a, s = model.rpn_head.assigner, model.rpn_head.sampler
    assert (a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou, a.match_low_quality) == (0.7, 0.3, 0.3, True)
    assert (s.num, s.pos_fraction, s.add_gt_as_proposals) == (256, 0.5, False)
    a, s = model.roi_head.bbox_assigner, model.roi_head.bbox_sampler
    assert (a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou, a.match_low_quality) == (0.5, 0.5, 0.5, False)
    assert (s.num, s.pos_fraction, s.add_gt_as_proposals) == (512, 0.25, True)
    assert model.test_cfg.rcnn.nms.iou_threshold == 0.5 and model.test_cfg.rpn.max_per_img == 1000
    assert model.train_cfg.rpn_proposal.nms_pre == 2000 and model.train_cfg.rpn_proposal.max_per_img == 1000
    # both device paths cover the recipe, and the proposal stage accepts the baseline's sizes (800 x 1344)
    assert model.rpn_head.device_train_ok() and model.roi_head.device_train_ok() and model._device_path_ok()
    full = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    model.rpn_head._check_proposal_limits(model.train_cfg.rpn_proposal, full)
    model.rpn_head._check_proposal_limits(model.test_cfg.rpn, full)


def test_parameter_names_and_shapes_are_the_references(model, gold):
    sd = model.state_dict()
    # (as a mapping: the order in which modules register their parameters is not part of a checkpoint)
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want


def test_other_heads_of_the_family_build_with_the_references_names():
    h = build_head(dict(type='RPNHead', in_channels=16, feat_channels=8, num_convs=2))
    assert [k for k in h.state_dict()] == ['rpn_conv.0.conv.weight', 'rpn_conv.0.conv.bias', 'rpn_conv.1.conv.weight',
                                           'rpn_conv.1.conv.bias', 'rpn_cls.weight', 'rpn_cls.bias', 'rpn_reg.weight',
                                           'rpn_reg.bias']
    h = build_head(dict(type='BBoxHead', in_channels=8, roi_feat_size=7, num_classes=3, reg_class_agnostic=True))
    assert {k: tuple(v.shape) for k, v in h.state_dict().items()} == {
        'fc_cls.weight': (4, 392), 'fc_cls.bias': (4,), 'fc_reg.weight': (4, 392), 'fc_reg.bias': (4,)}
    h = build_head(dict(type='Shared4Conv1FCBBoxHead', in_channels=8, conv_out_channels=8, fc_out_channels=16,
                        num_classes=3))
    assert len(h.shared_convs) == 4 and len(h.shared_fcs) == 1 and h.fc_reg.out_features == 12
    h = build_head(dict(type='ConvFCBBoxHead', in_channels=8, num_shared_fcs=1, num_cls_fcs=1, num_reg_fcs=1,
                        fc_out_channels=16, num_classes=3))
    assert len(h.cls_fcs) == len(h.reg_fcs) == 1
    with pytest.raises(TypeError):
        build_head(dict(type='Shared2FCBBoxHead', in_channels=8, num_classes=3, focal_reg=True))


def test_refused_configurations_raise(model):
    with pytest.raises(NotImplementedError, match='use_sigmoid=False'):
        build_head(ConfigDict(fi.rpn_head_cfg(loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))))
    imgs = [torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 64, 96)]
    metas = [fi.metas(1), [dict(fi.metas(1)[0], flip=True, flip_direction='horizontal')]]
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.roi_head.aug_test(None, None, metas)
    rpn = model.rpn_head
    with pytest.raises(ValueError, match='nms_pre'):
        rpn._check_proposal_limits(ConfigDict(nms_pre=5000, max_per_img=1000, nms=dict(type='nms', iou_threshold=0.7),
                                              min_bbox_size=0), fi.SIZES)
    with pytest.raises(ValueError, match='candidates'):
        rpn._check_proposal_limits(ConfigDict(nms_pre=4000, max_per_img=1000, nms=dict(type='nms', iou_threshold=0.7),
                                              min_bbox_size=0), [(200, 336)] * 5)
    with pytest.raises(NotImplementedError):
        build_head(ConfigDict(fi.roi_head_cfg(), mask_head=dict(type='FCNMaskHead')))


# ------------------------------------------------------------------------------------------- host path vs the fixture
def test_rpn_loss_host_path_reproduces_the_reference(gold):
    seed = int(gold['seed_rpnloss'])
    head = build_head(ConfigDict(fi.rpn_head_cfg())).train()
    cls, reg = fi.rpn_outputs(seed, grad=True)
    gt_bboxes, _ = fi.gts(seed)
    torch.manual_seed(seed + 100)
    losses = head.loss(cls, reg, gt_bboxes, fi.metas())
    for b, (pos, neg) in enumerate(head.last_drawn):        # the draw: the reference's calls in the reference's order
        assert pos.tolist() == gold[f'rpnloss_pos{b}'].tolist() and neg.tolist() == gold[f'rpnloss_neg{b}'].tolist()
    for k in ('loss_rpn_cls', 'loss_rpn_bbox'):
        got = torch.stack(losses[k]).detach().numpy()
        assert np.allclose(got, gold['rpnloss_' + k], rtol=1e-5, atol=1e-7), (k, got, gold['rpnloss_' + k])
    sum(losses['loss_rpn_cls'] + losses['loss_rpn_bbox']).backward()
    assert all(torch.isfinite(t.grad).all() for t in cls + reg)


def _roi_head_forward_cpu(rh, feats, rois):
    """the box head's forward from CPU pieces: RoIAlign of the C oracle per level, the FCs in torch"""
    ex = rh.bbox_roi_extractor
    lv = ex.map_roi_levels(rois, ex.num_inputs)
    out = torch.zeros(len(rois), ex.out_channels, 7, 7)
    for i, stride in enumerate(ex.featmap_strides):
        m = lv == i
        if m.any():
            out[m] = orc.roi_align_forward(feats[i].contiguous(), rois[m].contiguous(), 7, 1.0 / stride, 0, 'avg', True)
    x = out.flatten(1)
    for fc in rh.bbox_head.shared_fcs:
        x = F.relu(fc(x))
    return rh.bbox_head.fc_cls(x), rh.bbox_head.fc_reg(x)


def test_bbox_head_loss_host_path_reproduces_the_reference(gold):
    seed = int(gold['seed_std'])
    rh = build_head(ConfigDict(fi.roi_head_cfg()))
    rh.load_state_dict(util.seeded_state_dict(rh, seed=seed))
    feats, metas, gts, gls, props = fi.roi_inputs(seed)
    torch.manual_seed(seed + 100)
    samples = []
    for b in range(2):
        ar = rh.bbox_assigner.assign(props[b], gts[b], None, gls[b])
        samples.append(rh.bbox_sampler.sample(ar, props[b], gts[b], gls[b]))
    rois = core.bbox2roi([s.bboxes for s in samples])
    with torch.no_grad():
        cls_score, bbox_pred = _roi_head_forward_cpu(rh, feats, rois)
    targets = rh.bbox_head.get_targets(samples, gts, gls, rh.train_cfg)
    losses = rh.bbox_head.loss(cls_score, bbox_pred, rois, *targets)
    for k in ('loss_cls', 'loss_bbox', 'acc'):
        want = gold['std_train_' + k].reshape(-1)
        assert np.allclose(losses[k].reshape(-1).numpy(), want, rtol=1e-4, atol=1e-6), (k, losses[k], want)


# ------------------------------------------------------------------------------------------- float64 reference pinned
def _rpn_case(gold):
    seed = int(gold['seed_rpnloss'])
    head = build_head(ConfigDict(fi.rpn_head_cfg()))
    cls, reg = fi.rpn_outputs(seed)
    gt_bboxes, _ = fi.gts(seed)
    anchors = torch.cat(head.anchor_generator.grid_anchors(fi.SIZES, 'cpu'))
    gt_inds = torch.stack([head.assigner.assign(anchors, g, None, None).gt_inds for g in gt_bboxes])
    offs = [0, len(gt_bboxes[0]), len(gt_bboxes[0]) + len(gt_bboxes[1])]
    drawn = [np.concatenate([gold[f'rpnloss_pos{b}'], gold[f'rpnloss_neg{b}']]) for b in range(2)]
    total = sum(max(len(gold[f'rpnloss_pos{b}']), 1) + max(len(gold[f'rpnloss_neg{b}']), 1) for b in range(2))
    return head, cls, reg, anchors, gt_inds, torch.cat(gt_bboxes), offs, drawn, total


def test_float64_reference_agrees_with_the_fixture(gold):
    head, cls, reg, anchors, gt_inds, gts, offs, drawn, total = _rpn_case(gold)
    x, p = R.flatten_outputs([c.numpy() for c in cls], [r.numpy() for r in reg])
    ref = R.sampled_rpn_loss(x, p, anchors.numpy(), gt_inds.numpy(), gts.numpy(), offs, drawn, total)
    tol_c, tol_b = R.loss_tolerance(ref)
    want_c, want_b = gold['rpnloss_loss_rpn_cls'].astype(np.float64).sum(), gold['rpnloss_loss_rpn_bbox'].astype(np.float64).sum()
    # the fixture is ONE fp32 evaluation of the same sums (per level, then five values added here): it sits within the
    # fp32 bound of the float64 value, plus the rounding of the five stored numbers
    assert ref['n_cls'] == 512 and ref['n_bbox'] == 4 * sum(len(gold[f'rpnloss_pos{b}']) for b in range(2)) > 0
    assert abs(ref['loss_cls'] - want_c) <= tol_c + 8 * EPS32 * abs(want_c), (ref['loss_cls'], want_c, tol_c)
    assert abs(ref['loss_bbox'] - want_b) <= tol_b + 8 * EPS32 * abs(want_b), (ref['loss_bbox'], want_b, tol_b)
    # and its gradient against torch autograd in float64 on the host path's own formulas
    xt = torch.tensor(x, requires_grad=True)
    pt = torch.tensor(p, requires_grad=True)
    lc = lb = 0.0
    for b in range(2):
        idx = torch.as_tensor(drawn[b], dtype=torch.long)
        pos = (gt_inds[b][idx] > 0)
        lc = lc + F.binary_cross_entropy_with_logits(xt[b, idx], pos.double(), reduction='sum')
        pi = idx[pos]
        t = core.bbox2delta(anchors[pi].double(), gts[offs[b] + gt_inds[b][pi].long() - 1].double())
        lb = lb + (pt[b, pi] - t).abs().sum()
    ((lc + lb) / total).backward()
    assert np.allclose(ref['dx'], xt.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(ref['dpred'], pt.grad.numpy(), rtol=1e-12, atol=1e-15)
