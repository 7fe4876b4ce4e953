"""Seeded inputs and configurations shared by the FCOS baseline tests and the generator of their fixture
(tests/golden/make_golden_fcos.py -> g28_fcos.npz).  Inputs are regenerated from the seeds recorded in the fixture; the
fixture stores what the reference computed from them."""
import copy
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'fcos', 'fcos_r50_caffe_fpn_gn-head_1x_utdac.py')
H, W = 128, 192                                             # padded input: the smallest at which the stride-128 level has a
SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]         # point inside the image, (64, 64)
STRIDES = [8, 16, 32, 64, 128]
INF = 1e8
RANGES = ((-1, 16), (16, 32), (32, 64), (64, 96), (96, INF))    # the recipe's regress ranges scaled to the small input
SCALES = (1.0, 0.9, 1.1, 1.2, 0.8)                          # per-level Scale values of the head-level sections
POINTS = sum(h * w for h, w in SIZES)                       # 512 per image
TRAIN_NUM_GT = 3
BIG_BOX = (0.0, 0.0, 192.0, 128.0)                          # makes (64, 64) a positive of the top level
RADIUS = 0.75                                               # a center_sample_radius at which the label maps change
# nms_pre=50: three levels (384 / 96 / 24 points) go through the select, two (6 / 2) pass whole
TEST_CFG = dict(nms_pre=50, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=20)
CLASS_COUNTS = (4, 1, 3)
# the two variants the reference ships: fcos_r50_caffe_fpn_gn-head and fcos_center-normbbox-centeronreg-giou
VARIANTS = {
    'iou': dict(),
    'giou': dict(center_sampling=True, center_sample_radius=RADIUS, norm_on_bbox=True, centerness_on_reg=True,
                 loss_bbox=dict(type='GIoULoss', loss_weight=1.0)),
}


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end: the small test cfg and the scaled regress ranges"""
    m = model_cfg()
    m['test_cfg'] = copy.deepcopy(TEST_CFG)
    m['bbox_head']['regress_ranges'] = RANGES
    return m


def head_cfg(num_classes=4, **over):
    """the recipe's FCOSHead, small (64 channels, 2 tower convs), with the small test cfg, as build_head takes it"""
    m = model_cfg()
    cfg = copy.deepcopy(m['bbox_head'])
    cfg.update(num_classes=num_classes, in_channels=64, feat_channels=64, stacked_convs=2, regress_ranges=RANGES,
               train_cfg=copy.deepcopy(m['train_cfg']), test_cfg=copy.deepcopy(TEST_CFG))
    cfg.update(copy.deepcopy(over))
    return cfg


def metas(batch=2):
    """images of different real sizes inside the (H, W) pad and different scale factors: per-image clip border, rescale"""
    shapes = [(H, W - 3), (H - 7, W - 20), (H - 2, W)]
    scales = [[1.1, 1.2, 1.1, 1.2], [0.8, 0.75, 0.8, 0.75], [1.0, 1.0, 1.0, 1.0]]
    return [{'img_shape': shapes[b % 3] + (3,), 'ori_shape': shapes[b % 3] + (3,), 'pad_shape': (H, W, 3),
             'scale_factor': np.array(scales[b % 3], dtype=np.float32), 'flip': False, 'filename': '<demo>.png'}
            for b in range(batch)]


def head_outputs(seed, num_classes=4, batch=2, norm_on_bbox=False, empty=False, grad=False):
    """seeded RAW head outputs, reference layout per level: cls (B, C, h, w), raw distances (B, 4, h, w) BEFORE Scale and
    exp / relu, centerness (B, 1, h, w).  Class logits around -4 (about one class score in seven passes score_thr = 0.05);
    raw distances so that exp(scale * raw) is about 1.5 strides, or under norm_on_bbox about one (stride-normalised) unit
    with one value in six negative, so that the relu branch runs.  `empty`: no class score of image 1 reaches the
    threshold."""
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(batch, num_classes, h, w, generator=g) * 2 - 4 for h, w in SIZES]
    if norm_on_bbox:
        raw = [torch.randn(batch, 4, h, w, generator=g) + 1.0 for h, w in SIZES]
    else:
        raw = [torch.randn(batch, 4, h, w, generator=g) * 0.5 + float(np.log(1.5 * s)) for (h, w), s in zip(SIZES, STRIDES)]
    ctr = [torch.randn(batch, 1, h, w, generator=g) for h, w in SIZES]
    if empty:
        for c in cls:
            c[1] = c[1] * 0.25 - 4.0             # logits -5 +- 0.5, all distinct: sigmoid(-3.5) = 0.029 < score_thr
    if grad:
        cls, raw, ctr = ([t.requires_grad_() for t in lst] for lst in (cls, raw, ctr))
    return cls, raw, ctr


def decoded(raw, scales, norm_on_bbox, training):
    """what the head's forward makes of the raw distances (Scale, then exp, or relu [* stride at test time]): the
    `bbox_preds` the reference-signature `loss` / `get_bboxes` take"""
    out = []
    for r, s, stride in zip(raw, scales, STRIDES):
        d = r * s
        if norm_on_bbox:
            d = torch.relu(d)
            d = d if training else d * stride
        else:
            d = d.exp()
        out.append(d)
    return out


def gts(seed, num_gt=TRAIN_NUM_GT, batch=2, num_classes=4):
    """ground truth of the (H, W) demo batch (tests/util.demo_inputs) plus the hand-placed large box in every image (class
    0), without which the stride-128 level has no positive at these regress ranges"""
    from tests import util
    _, _, gt_bboxes, gt_labels = util.demo_inputs(batch, H, W, num_classes=num_classes, seed=seed, num_gt=num_gt)
    gt_bboxes = [torch.cat([b, b.new_tensor([BIG_BOX])]) for b in gt_bboxes]
    gt_labels = [torch.cat([l, l.new_zeros(1)]) for l in gt_labels]
    return gt_bboxes, gt_labels


def fixture_state_dict(model, seed):
    """tests/util.seeded_state_dict, conditioned for the FCOS head: class logits lowered so that a few dozen candidates
    per image pass score_thr, and distance weights of the size a trained head produces (exp of an O(1) value)"""
    from tests import util
    sd = util.seeded_state_dict(model, seed=seed)
    for k in ('bbox_head.conv_reg.weight', 'bbox_head.conv_cls.weight', 'bbox_head.conv_centerness.weight'):
        if k in sd:
            sd[k] = sd[k] / 8.0
    if 'bbox_head.conv_reg.bias' in sd:
        sd['bbox_head.conv_reg.bias'] = sd['bbox_head.conv_reg.bias'] * 0 + 2.5
        sd['bbox_head.conv_cls.bias'] = sd['bbox_head.conv_cls.bias'] * 0 - 3.0
    return sd
