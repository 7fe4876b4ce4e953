"""Seeded inputs and configurations shared by the Faster R-CNN baseline tests and the generator of their fixture
(tests/golden/make_golden_faster_rcnn.py -> g25_faster_rcnn.npz).  Inputs are regenerated from the seeds recorded in
the fixture; the fixture stores what the reference computed from them."""
import copy
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'faster_rcnn', 'faster_rcnn_r50_fpn_1x_utdac.py')
BOOST_CONFIG = os.path.join(ROOT, 'configs', 'boosting_rcnn', 'boosting_rcnn_r50_pafpn_1x_utdac.py')
H, W = 64, 96                                           # padded input; img_shape is (H, W - 3)
SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]     # strides 4 .. 64
A = 3
TRAIN_NUM_GT = 3                                        # ground truths per image of the train iterations
_NMS07 = dict(type='nms', iou_threshold=0.7)
# nms_pre=50: the three finer levels (1152 / 288 / 72 anchors) are selected, the two coarser (18 / 6) pass through
PROPOSAL_CFGS = {
    'train': dict(nms_pre=50, max_per_img=40, nms=_NMS07, min_bbox_size=0),
    'test': dict(nms_pre=50, max_per_img=20, nms=_NMS07, min_bbox_size=0),
    'minsize': dict(nms_pre=50, max_per_img=40, nms=_NMS07, min_bbox_size=12),
    # with `empty=True` outputs: image 1's boxes all shrink below min_bbox_size, nothing of it survives
    'empty': dict(nms_pre=50, max_per_img=40, nms=_NMS07, min_bbox_size=12),
}


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def small_proposals(m):
    """a detector cfg with the proposal counts of PROPOSAL_CFGS: at the recipe's own counts (1000 per level) a 64 x 96
    input yields ~10^6 candidate pairs per image, and some pair always sits within the generator's IoU margin"""
    m = copy.deepcopy(m)
    m['train_cfg']['rpn_proposal'] = copy.deepcopy(PROPOSAL_CFGS['train'])
    m['test_cfg']['rpn'] = copy.deepcopy(PROPOSAL_CFGS['test'])
    return m


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end"""
    return small_proposals(model_cfg())


def rpn_head_cfg(**over):
    """the recipe's RPNHead with its train / test cfg, as build_head takes it"""
    m = model_cfg()
    cfg = copy.deepcopy(m['rpn_head'])
    cfg.update(train_cfg=copy.deepcopy(m['train_cfg']['rpn']), test_cfg=copy.deepcopy(m['test_cfg']['rpn']))
    cfg.update(over)
    return cfg


def roi_head_cfg(kind='StandardRoIHead'):
    """head-level second stage on the 5-level seeded pyramid of tests/util.variant_inputs (strides 8 .. 128)"""
    from brcnn import Config
    if kind == 'StandardRoIHead':
        m = model_cfg()
    else:
        m = Config.fromfile(BOOST_CONFIG).model.to_dict()
    cfg = copy.deepcopy(m['roi_head'])
    cfg['bbox_roi_extractor']['featmap_strides'] = [8, 16, 32, 64]
    cfg.update(train_cfg=copy.deepcopy(m['train_cfg']['rcnn']), test_cfg=copy.deepcopy(m['test_cfg']['rcnn']))
    return cfg


def cross_model_cfg(which):
    """the ablation's two mixes as detector configs: 'atss_std' = the boosting recipe with the standard second stage,
    'rpn_prob' = the baseline recipe with the boosting second stage"""
    from brcnn import Config
    base, boost = model_cfg(), Config.fromfile(BOOST_CONFIG).model.to_dict()
    if which == 'atss_std':
        m = copy.deepcopy(boost)
        m['roi_head'] = copy.deepcopy(base['roi_head'])
        m['roi_head']['bbox_roi_extractor']['featmap_strides'] = [8, 16, 32, 64]
        m['train_cfg']['rcnn'] = copy.deepcopy(base['train_cfg']['rcnn'])
        m['test_cfg']['rcnn'] = copy.deepcopy(base['test_cfg']['rcnn'])
    elif which == 'rpn_prob':
        m = copy.deepcopy(base)
        m['roi_head'] = copy.deepcopy(boost['roi_head'])
        m['roi_head']['bbox_roi_extractor']['featmap_strides'] = [4, 8, 16, 32]
        m['train_cfg']['rcnn'] = copy.deepcopy(boost['train_cfg']['rcnn'])
        m['test_cfg']['rcnn'] = copy.deepcopy(boost['test_cfg']['rcnn'])
    else:
        raise KeyError(which)
    return small_proposals(m)


def metas(batch=2):
    return [{'img_shape': (H, W - 3, 3), 'ori_shape': (H, W - 3, 3), 'pad_shape': (H, W, 3),
             'scale_factor': np.array([1.1, 1.2, 1.1, 1.2], dtype=np.float32), 'flip': False,
             'filename': '<demo>.png'} for _ in range(batch)]


def rpn_outputs(seed, batch=2, empty=False, grad=False):
    """seeded RPN head outputs, reference layout: cls (B, A, h, w), reg (B, 4A, h, w) per level"""
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(batch, A, h, w, generator=g) * 2 for h, w in SIZES]
    reg = [torch.randn(batch, 4 * A, h, w, generator=g) * 0.5 for h, w in SIZES]
    if empty:
        for r in reg:
            r.view(batch, A, 4, *r.shape[2:])[1, :, 2:] = -10.0        # dw, dh of image 1: clamped to the ratio clip
    if grad:
        cls, reg = [t.requires_grad_() for t in cls], [t.requires_grad_() for t in reg]
    return cls, reg


def gts(seed, num_gt=TRAIN_NUM_GT, batch=2):
    """ground truth of the (H, W) demo batch (tests/util.demo_inputs)"""
    from tests import util
    _, _, gt_bboxes, gt_labels = util.demo_inputs(batch, H, W, num_classes=4, seed=seed, num_gt=num_gt)
    return gt_bboxes, gt_labels


def roi_inputs(seed, num_classes=4):
    """head-level second-stage inputs: tests/util.variant_inputs with every 8th proposal (about 40 per image, so that
    the candidate pairs of the class-wise NMS can all keep the generator's IoU margin)"""
    from tests import util
    feats, vmetas, vg, vl, props = util.variant_inputs(num_classes, 1, seed)
    return feats, vmetas, vg, vl, [p[::8].contiguous() for p in props]


def fixture_state_dict(model, seed):
    """tests/util.seeded_state_dict, conditioned for the plain heads: the seeded pyramid has a standard deviation of ~30
    (nothing normalises it, as the GroupNorm tower of the RetinaRPN does), which saturates the sigmoid / softmax scores
    to exactly 1.0 and leaves the order of detections to ties.  The first layer of each head is scaled down so that
    logits are O(1)."""
    from tests import util
    sd = util.seeded_state_dict(model, seed=seed)
    for k in ('rpn_head.rpn_conv.weight', 'roi_head.bbox_head.shared_fcs.0.weight'):
        if k in sd:
            sd[k] = sd[k] / 30.0
    # proposal deltas of the size a trained RPN produces (~0.1 instead of ~0.5 of an anchor that is up to 512 px wide):
    # every px of a box carries the deltas' round-off times the anchor size, in the reference's fp32 run as on the device
    if 'rpn_head.rpn_reg.weight' in sd:
        sd['rpn_head.rpn_reg.weight'] = sd['rpn_head.rpn_reg.weight'] / 4.0
    return sd
