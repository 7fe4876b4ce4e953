"""Seeded inputs and configurations shared by the ATSS baseline tests and the generator of their fixture
(tests/golden/make_golden_atss.py -> g29_atss.npz).  Inputs are regenerated from the seeds recorded in the fixture; the
fixture stores what the reference computed from them."""
import copy
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, 'configs', 'atss', 'atss_r50_fpn_1x_utdac.py')
H, W = 128, 192                                             # the padded input of the FCOS tests
SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
STRIDES = [8, 16, 32, 64, 128]
# the head-level sections use anchors of 2 strides (16 .. 256 px): at the recipe's 8 every positive of a 128 x 192 input
# lands on level 0
OCTAVE = 2
TOPK = 9
MEANS, STDS = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
SCALES = (1.0, 0.9, 1.1, 1.2, 0.8)                          # per-level Scale values of the head-level sections
ANCHORS = sum(h * w for h, w in SIZES)                      # 512 per image
TRAIN_NUM_GT = 3
BIG_BOX = (0.0, 0.0, 192.0, 128.0)                          # the whole image: positives on the coarse levels
# nms_pre=50: two levels (384 / 96 anchors) go through the select, three (24 / 6 / 2) pass whole
TEST_CFG = dict(nms_pre=50, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6), max_per_img=20)
CLASS_COUNTS = (4, 1)


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end: the small test cfg"""
    m = model_cfg()
    m['test_cfg'] = copy.deepcopy(TEST_CFG)
    return m


def head_cfg(num_classes=4, **over):
    """the recipe's ATSSHead, small (64 channels, 2 tower convs, anchors of OCTAVE strides), with the small test cfg, as
    build_head takes it"""
    m = model_cfg()
    cfg = copy.deepcopy(m['bbox_head'])
    cfg.update(num_classes=num_classes, in_channels=64, feat_channels=64, stacked_convs=2,
               train_cfg=copy.deepcopy(m['train_cfg']), test_cfg=copy.deepcopy(TEST_CFG))
    cfg['anchor_generator']['octave_base_scale'] = OCTAVE
    cfg.update(copy.deepcopy(over))
    return cfg


def metas(batch=2, pads=None):
    """images of different real sizes inside the (H, W) pad and different scale factors: per-image clip border, rescale.
    `pads`: per-image pad_shape (h, w) smaller than the batch pad (cells beyond it are invalid)"""
    shapes = [(H, W - 3), (H - 7, W - 20), (H - 2, W)]
    scales = [[1.1, 1.2, 1.1, 1.2], [0.8, 0.75, 0.8, 0.75], [1.0, 1.0, 1.0, 1.0]]
    out = []
    for b in range(batch):
        pad = (H, W) if pads is None else tuple(pads[b])
        shape = (min(shapes[b % 3][0], pad[0]), min(shapes[b % 3][1], pad[1]))
        out.append({'img_shape': shape + (3,), 'ori_shape': shape + (3,), 'pad_shape': pad + (3,),
                    'scale_factor': np.array(scales[b % 3], dtype=np.float32), 'flip': False, 'filename': '<demo>.png'})
    return out


def head_outputs(seed, num_classes=4, batch=2, empty=False, grad=False):
    """seeded RAW head outputs, reference layout per level: cls (B, C, h, w), raw deltas (B, 4, h, w) BEFORE the Scale,
    centerness (B, 1, h, w).  Class logits around -4 (about one class score in seven passes score_thr = 0.05); raw deltas
    of standard deviation 2: the centre moves by about 0.2 anchor sizes, the size changes by a factor of about e^0.4.
    `empty`: no class score of image 1 reaches the threshold."""
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(batch, num_classes, h, w, generator=g) * 2 - 4 for h, w in SIZES]
    raw = [torch.randn(batch, 4, h, w, generator=g) * 2 for h, w in SIZES]
    ctr = [torch.randn(batch, 1, h, w, generator=g) for h, w in SIZES]
    if empty:
        for c in cls:
            c[1] = c[1] * 0.25 - 4.0             # logits -5 +- 0.5, all distinct: sigmoid(-3.5) = 0.029 < score_thr
    if grad:
        cls, raw, ctr = ([t.requires_grad_() for t in lst] for lst in (cls, raw, ctr))
    return cls, raw, ctr


def scaled(raw, scales):
    """what the head's forward makes of the raw deltas (the per-level Scale): the `bbox_preds` the reference-signature
    `loss` / `get_bboxes` take"""
    return [r * s for r, s in zip(raw, scales)]


def gts(seed, num_gt=TRAIN_NUM_GT, batch=2, num_classes=4):
    """ground truth of the (H, W) demo batch (tests/util.demo_inputs) plus the whole-image box in every image (class 0)"""
    from tests import util
    _, _, gt_bboxes, gt_labels = util.demo_inputs(batch, H, W, num_classes=num_classes, seed=seed, num_gt=num_gt)
    gt_bboxes = [torch.cat([b, b.new_tensor([BIG_BOX])]) for b in gt_bboxes]
    gt_labels = [torch.cat([l, l.new_zeros(1)]) for l in gt_labels]
    return gt_bboxes, gt_labels


def fixture_state_dict(model, seed):
    """tests/util.seeded_state_dict, conditioned for the ATSS head: class logits lowered so that a few dozen candidates
    per image pass score_thr, delta weights of the size a trained head produces"""
    from tests import util
    sd = util.seeded_state_dict(model, seed=seed)
    for k in ('bbox_head.atss_reg.weight', 'bbox_head.atss_cls.weight', 'bbox_head.atss_centerness.weight'):
        if k in sd:
            sd[k] = sd[k] / 8.0
    if 'bbox_head.atss_cls.bias' in sd:
        sd['bbox_head.atss_cls.bias'] = sd['bbox_head.atss_cls.bias'] * 0 - 3.0
    return sd
