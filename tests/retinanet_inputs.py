"""Seeded inputs and configurations shared by the RetinaNet baseline tests and the generator of their fixture
(tests/golden/make_golden_retinanet.py -> g27_retinanet.npz).  Inputs are regenerated from the seeds recorded in the
fixture; the fixture stores what the reference computed from them."""
import copy
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'retinanet', 'retinanet_r50_fpn_1x_utdac.py')
H, W = 64, 96                                           # padded input
SIZES = [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]       # strides 8 .. 128
STRIDES = [8, 16, 32, 64, 128]
A = 9
TRAIN_NUM_GT = 3
# nms_pre=50: the three finer levels (864 / 216 / 54 anchors) are selected, the two coarser (18 / 9) pass through whole
TEST_CFG = dict(nms_pre=50, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=20)
CLASS_COUNTS = (4, 1, 3)


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end: at the recipe's own nms_pre (1000 per level) a 64 x 96 input yields
    so many candidate pairs that some pair always sits within the generator's IoU margin"""
    m = model_cfg()
    m['test_cfg'] = copy.deepcopy(TEST_CFG)
    return m


def head_cfg(num_classes=4, **over):
    """the recipe's RetinaHead with its train cfg and the small test cfg, as build_head takes it"""
    m = model_cfg()
    cfg = copy.deepcopy(m['bbox_head'])
    cfg.update(num_classes=num_classes, train_cfg=copy.deepcopy(m['train_cfg']), test_cfg=copy.deepcopy(TEST_CFG))
    cfg.update(over)
    return cfg


def metas(batch=2):
    """images of different real sizes inside the (H, W) pad and different scale factors: per-image clip border, rescale"""
    shapes = [(H, W - 3), (H - 7, W - 20), (H - 2, W)]
    scales = [[1.1, 1.2, 1.1, 1.2], [0.8, 0.75, 0.8, 0.75], [1.0, 1.0, 1.0, 1.0]]
    return [{'img_shape': shapes[b % 3] + (3,), 'ori_shape': shapes[b % 3] + (3,), 'pad_shape': (H, W, 3),
             'scale_factor': np.array(scales[b % 3], dtype=np.float32), 'flip': False, 'filename': '<demo>.png'}
            for b in range(batch)]


def head_outputs(seed, num_classes=4, batch=2, empty=False, grad=False):
    """seeded head outputs, reference layout: cls (B, A*C, h, w), reg (B, 4A, h, w) per level.  `empty`: no class score
    of image 1 reaches the score threshold.  Logits around -6: about one class score in sixteen passes score_thr = 0.05, a
    few dozen candidates per image -- few enough pairs for the generator's IoU margin to hold on some seed"""
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(batch, A * num_classes, h, w, generator=g) * 2 - 6 for h, w in SIZES]
    reg = [torch.randn(batch, 4 * A, h, w, generator=g) * 0.5 for h, w in SIZES]
    if empty:
        for c in cls:
            c[1] = c[1] * 0.5 - 5.0              # logits -8 +- 1, all distinct: sigmoid(-4) = 0.018 < score_thr
    if grad:
        cls, reg = [t.requires_grad_() for t in cls], [t.requires_grad_() for t in reg]
    return cls, reg


def gts(seed, num_gt=TRAIN_NUM_GT, batch=2, num_classes=4):
    """ground truth of the (H, W) demo batch (tests/util.demo_inputs)"""
    from tests import util
    _, _, gt_bboxes, gt_labels = util.demo_inputs(batch, H, W, num_classes=num_classes, seed=seed, num_gt=num_gt)
    return gt_bboxes, gt_labels


def fixture_state_dict(model, seed):
    """tests/util.seeded_state_dict, conditioned for the un-normalised towers: the seeded pyramid has a standard deviation
    of ~30, which four plain convs amplify until every sigmoid saturates to exactly 0 or 1 and the order of detections is
    left to ties.  The first layer of each tower is scaled down so that logits are O(1), and the box deltas are of the
    size a trained head produces (every px of a box carries the deltas' round-off times the anchor size)."""
    from tests import util
    sd = util.seeded_state_dict(model, seed=seed)
    for k in ('bbox_head.cls_convs.0.conv.weight', 'bbox_head.reg_convs.0.conv.weight'):
        if k in sd:
            sd[k] = sd[k] / 30.0
    if 'bbox_head.retina_reg.weight' in sd:
        sd['bbox_head.retina_reg.weight'] = sd['bbox_head.retina_reg.weight'] / 4.0
    return sd
