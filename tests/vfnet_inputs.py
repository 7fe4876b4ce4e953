"""Seeded inputs and configurations shared by the VFNet baseline tests and the generator of their fixture
(tests/golden/make_golden_vfnet.py -> g31_vfnet.npz), on the pyramid of tests/atss_inputs.py (128 x 192 input, levels 16 x 24 ..
1 x 2, 2 images), whose metas and test cfg are used as they are.  Inputs are regenerated from the seeds recorded in the
fixture; the fixture stores what the reference computed from them."""
import copy
import os

import torch

from tests import atss_inputs as ai
from tests import gfl_inputs as gi

ROOT = ai.ROOT
CONFIG = os.path.join(ROOT, 'configs', 'vfnet', 'vfnet_r50_fpn_1x_utdac.py')
H, W, SIZES, STRIDES, OCTAVE, TOPK = ai.H, ai.W, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK
SCALES, ANCHORS, TRAIN_NUM_GT, TEST_CFG, CLASS_COUNTS = ai.SCALES, ai.ANCHORS, ai.TRAIN_NUM_GT, ai.TEST_CFG, ai.CLASS_COUNTS
SCALES_REFINE = (1.1, 1.0, 0.9, 1.05, 0.95)
REG_DENOMS = [64, 128, 256, 512, 1024]                      # the upper regress ranges; the last is twice the one before
GRADIENT_MUL = 0.1
metas = ai.metas
gts = gi.gts                                                # the demo boxes plus a non-integer box over nearly the whole image


def rows(batch=2):
    return batch * ANCHORS


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end: the small test cfg"""
    m = model_cfg()
    m['test_cfg'] = copy.deepcopy(TEST_CFG)
    return m


def head_cfg(num_classes=4, **over):
    """the recipe's VFNetHead, small (64 channels, 2 tower convs, anchors of OCTAVE strides), with the small test cfg, as
    build_head takes it"""
    m = model_cfg()
    cfg = copy.deepcopy(m['bbox_head'])
    cfg.update(num_classes=num_classes, in_channels=64, feat_channels=64, stacked_convs=2,
               anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=OCTAVE, scales_per_octave=1,
                                     center_offset=0.0, strides=list(STRIDES)),
               train_cfg=copy.deepcopy(m['train_cfg']), test_cfg=copy.deepcopy(TEST_CFG))
    cfg.update(copy.deepcopy(over))
    return cfg


def head_outputs(seed, num_classes=4, batch=2, empty=False, grad=False):
    """seeded RAW head outputs, reference layout per level: cls (B, C, h, w), raw0 (B, 4, h, w) the output of `vfnet_reg` and
    raw1 (B, 4, h, w) that of `vfnet_reg_refine`, both BEFORE their Scale.  Class logits around -4 (about one class score in
    seven passes score_thr = 0.05).  raw0 of mean -1.2 and standard deviation 0.6: first distances of about 0.3 reg_denom,
    boxes of 40 px on level 0 up to the whole image on level 2 and beyond it above; raw1 of standard deviation 0.3: refinement
    factors of 0.5 to 2.  `empty`: no class score of image 1 reaches the threshold."""
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(batch, num_classes, h, w, generator=g) * 2 - 4 for h, w in SIZES]
    raw0 = [torch.randn(batch, 4, h, w, generator=g) * 0.6 - 1.2 for h, w in SIZES]
    raw1 = [torch.randn(batch, 4, h, w, generator=g) * 0.3 for h, w in SIZES]
    if empty:
        for c in cls:
            c[1] = c[1] * 0.25 - 4.0             # logits -5 +- 0.5, all distinct: sigmoid(-3.5) = 0.029 < score_thr
    if grad:
        cls, raw0, raw1 = ([t.requires_grad_() for t in lst] for lst in (cls, raw0, raw1))
    return cls, raw0, raw1


def distances(raw0, raw1, scales=SCALES, scales_refine=SCALES_REFINE, denoms=REG_DENOMS):
    """what the head's forward makes of the raw outputs (vfnet_head.py:246-266): `bbox_preds` = exp(scale * raw0) *
    reg_denom and `bbox_preds_refine` = exp(scale_refine * raw1) * bbox_preds.detach(), the tensors the reference-signature
    `loss` / `get_bboxes` take"""
    d0 = [(r * s).float().exp() * d for r, s, d in zip(raw0, scales, denoms)]
    d1 = [(r * s).float().exp() * p.detach() for r, s, p in zip(raw1, scales_refine, d0)]
    return d0, d1


def features(seed, batch=2, channels=64, dtype=torch.float32):
    """a seeded pyramid for the head-level forward sections: (B, channels, h, w) per level"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(batch, channels, h, w, generator=g).to(dtype) for h, w in SIZES]


def small_feature(seed, channels=64, dtype=torch.float32):
    """one (1, channels, 6, 7) map for the sections that follow a gradient through the star offsets"""
    g = torch.Generator().manual_seed(seed + 7000)
    return torch.randn(1, channels, 6, 7, generator=g).to(dtype)


def seeded_head_state(head, seed):
    """seeded weights of a small head, conditioned like `fixture_state_dict`: Normal(0, 0.05) convs, GroupNorm weights near
    1; `vfnet_reg` / `vfnet_reg_refine` small, so that the first distances stay near reg_denom -- 64 px (8 cells) inside the
    16 x 24 map of level 0, 1024 px (8 cells) far outside the 1 x 2 map of level 4: both situations of the star sampling
    occur --, the class bias at -3"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in head.state_dict().items():
        if k.endswith('gn.weight'):
            sd[k] = 1 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith('.scale'):
            sd[k] = torch.ones(v.shape) + 0.1 * torch.randn(v.shape, generator=g)
        elif v.dim() == 4:
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = 0.05 * torch.randn(v.shape, generator=g)
    for k in ('vfnet_reg.weight', 'vfnet_reg_refine.weight', 'vfnet_cls.weight'):
        sd[k] = sd[k] / 4.0
    sd['vfnet_reg.bias'] = sd['vfnet_reg.bias'] * 0 - 0.5 + 0.2 * torch.randn(4, generator=g)
    sd['vfnet_cls.bias'] = sd['vfnet_cls.bias'] * 0 - 3.0
    return sd


def fixture_state_dict(model, seed):
    """tests/util.seeded_state_dict, conditioned for the VFNet head: class logits lowered so that a few dozen candidates per
    image pass score_thr; `vfnet_reg` / `vfnet_reg_refine` small with zero bias: D0 near reg_denom (see `seeded_head_state`)"""
    from tests import util
    sd = util.seeded_state_dict(model, seed=seed)
    for k in ('bbox_head.vfnet_reg.weight', 'bbox_head.vfnet_reg_refine.weight', 'bbox_head.vfnet_cls.weight'):
        if k in sd:
            sd[k] = sd[k] / 8.0
    for k in ('bbox_head.vfnet_reg.bias', 'bbox_head.vfnet_reg_refine.bias'):
        if k in sd:
            sd[k] = sd[k] * 0
    if 'bbox_head.vfnet_cls.bias' in sd:
        sd['bbox_head.vfnet_cls.bias'] = sd['bbox_head.vfnet_cls.bias'] * 0 - 3.0
    return sd
