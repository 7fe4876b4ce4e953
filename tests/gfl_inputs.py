"""Seeded inputs and configurations shared by the GFL baseline tests and the generator of their fixture
(tests/golden/make_golden_gfl.py -> g30_gfl.npz), on the pyramid of tests/atss_inputs.py (128 x 192 input, levels 16 x 24 ..
1 x 2, 2 images), whose metas and test cfg are used as they are.  Inputs are regenerated from the seeds
recorded in the fixture; the fixture stores what the reference computed from them."""
import copy
import os

import torch

from tests import atss_inputs as ai

ROOT = ai.ROOT
CONFIG = os.path.join(ROOT, 'configs', 'gfl', 'gfl_r50_fpn_1x_utdac.py')
H, W, SIZES, STRIDES, OCTAVE, TOPK = ai.H, ai.W, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK
SCALES, ANCHORS, TRAIN_NUM_GT, TEST_CFG, CLASS_COUNTS = ai.SCALES, ai.ANCHORS, ai.TRAIN_NUM_GT, ai.TEST_CFG, ai.CLASS_COUNTS
REG_MAX = 16
metas = ai.metas
# nearly the whole image: positives on the coarse levels.  Not the integer box of tests/atss_inputs.py: from the integer anchor
# centres its sides lie at whole numbers of strides, exactly on the bin edges of the Distribution Focal Loss
BIG_BOX = (1.3, 0.7, 190.6, 127.1)


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end: the small test cfg"""
    m = model_cfg()
    m['test_cfg'] = copy.deepcopy(TEST_CFG)
    return m


def head_cfg(num_classes=4, **over):
    """the recipe's GFLHead, small (64 channels, 2 tower convs, anchors of OCTAVE strides), with the small test cfg, as
    build_head takes it"""
    m = model_cfg()
    cfg = copy.deepcopy(m['bbox_head'])
    cfg.update(num_classes=num_classes, in_channels=64, feat_channels=64, stacked_convs=2,
               train_cfg=copy.deepcopy(m['train_cfg']), test_cfg=copy.deepcopy(TEST_CFG))
    cfg['anchor_generator']['octave_base_scale'] = OCTAVE
    cfg.update(copy.deepcopy(over))
    return cfg


def head_outputs(seed, num_classes=4, batch=2, empty=False, grad=False, reg_max=REG_MAX):
    """seeded RAW head outputs, reference layout per level: cls (B, C, h, w) and box logits (B, 4 * (reg_max + 1), h, w)
    BEFORE the Scale.  Class logits around -4 (about one class score in seven passes score_thr = 0.05).  Box logits of
    standard deviation 2 with a bump of 5 on one bin per (cell, side), the bin drawn towards the small distances (reg_max *
    u^2): distributions with a mode and a tail, expectations of 1 to 12 strides.  `empty`: no class score of image 1 reaches
    the threshold."""
    g = torch.Generator().manual_seed(seed)
    n = reg_max + 1
    cls = [torch.randn(batch, num_classes, h, w, generator=g) * 2 - 4 for h, w in SIZES]
    raw = []
    for h, w in SIZES:
        x = torch.randn(batch, 4, n, h, w, generator=g) * 2
        k = (torch.rand(batch, 4, 1, h, w, generator=g) ** 2 * reg_max).long()
        raw.append((x + 5.0 * torch.zeros_like(x).scatter_(2, k, 1.0)).reshape(batch, 4 * n, h, w))
    if empty:
        for c in cls:
            c[1] = c[1] * 0.25 - 4.0             # logits -5 +- 0.5, all distinct: sigmoid(-3.5) = 0.029 < score_thr
    if grad:
        cls, raw = ([t.requires_grad_() for t in lst] for lst in (cls, raw))
    return cls, raw


def gts(seed, num_gt=TRAIN_NUM_GT, batch=2, num_classes=4):
    """ground truth of the (H, W) demo batch (tests/util.demo_inputs) plus BIG_BOX in every image (class 0)"""
    from tests import util
    _, _, gt_bboxes, gt_labels = util.demo_inputs(batch, H, W, num_classes=num_classes, seed=seed, num_gt=num_gt)
    gt_bboxes = [torch.cat([b, b.new_tensor([BIG_BOX])]) for b in gt_bboxes]
    gt_labels = [torch.cat([l, l.new_zeros(1)]) for l in gt_labels]
    return gt_bboxes, gt_labels


def scaled(raw, scales):
    """what the head's forward makes of the raw box logits (the per-level Scale): the `bbox_preds` the reference-signature
    `loss` / `get_bboxes` take"""
    return [r * s for r, s in zip(raw, scales)]


def fixture_state_dict(model, seed):
    """tests/util.seeded_state_dict, conditioned for the GFL head: class logits lowered so that a few dozen candidates
    per image pass score_thr, box logits of the size a trained head produces"""
    from tests import util
    sd = util.seeded_state_dict(model, seed=seed)
    for k in ('bbox_head.gfl_reg.weight', 'bbox_head.gfl_cls.weight'):
        if k in sd:
            sd[k] = sd[k] / 8.0
    if 'bbox_head.gfl_cls.bias' in sd:
        sd['bbox_head.gfl_cls.bias'] = sd['bbox_head.gfl_cls.bias'] * 0 - 3.0
    if 'bbox_head.integral.project' in sd:
        sd['bbox_head.integral.project'] = torch.linspace(0, REG_MAX, REG_MAX + 1)
    return sd
