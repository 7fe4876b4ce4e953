"""Seeded inputs and configurations shared by the Cascade R-CNN baseline tests and the generator of their fixture
(tests/golden/make_golden_cascade_rcnn.py -> g26_cascade_rcnn.npz), beside tests/faster_rcnn_inputs.py, whose shapes,
metas and proposal counts they reuse.  Inputs are regenerated from the seeds recorded in the fixture; the fixture stores
what the reference computed from them."""
import copy
import os

import torch

from tests import faster_rcnn_inputs as fi

ROOT = fi.ROOT
CONFIG = os.path.join(ROOT, 'configs', 'cascade_rcnn', 'cascade_rcnn_r50_fpn_1x_utdac.py')
NUM_STAGES = 3
REFINE_C = 4                # classes of the seeded refinement rows (section a)
REFINE_ROWS = (37, 21)      # sampled rows per image there


def model_cfg():
    from brcnn import Config
    return Config.fromfile(CONFIG).model.to_dict()


def fixture_model_cfg():
    """the recipe as the fixture runs it end to end: the proposal counts of tests/faster_rcnn_inputs.py"""
    return fi.small_proposals(model_cfg())


def roi_head_cfg(**head_over):
    """head-level cascade on the 5-level seeded pyramid of tests/util.variant_inputs (strides 8 .. 128); `head_over`
    updates every stage's box head"""
    m = model_cfg()
    cfg = copy.deepcopy(m['roi_head'])
    cfg['bbox_roi_extractor']['featmap_strides'] = [8, 16, 32, 64]
    for h in cfg['bbox_head']:
        h.update(copy.deepcopy(head_over))
    cfg.update(train_cfg=copy.deepcopy(m['train_cfg']['rcnn']), test_cfg=copy.deepcopy(m['test_cfg']['rcnn']))
    return cfg


def box_head_cfg(stage=0, **over):
    """one stage's box head of the recipe, as build_head takes it"""
    cfg = copy.deepcopy(model_cfg()['roi_head']['bbox_head'][stage])
    cfg.update(over)
    return cfg


def _scale_first_layers(sd, prefix):
    """tests/faster_rcnn_inputs.fixture_state_dict's conditioning for every stage: the seeded pyramid has a standard
    deviation of ~30, which saturates the softmax; the first layer of each head is scaled down so that logits are O(1)"""
    for i in range(NUM_STAGES):
        k = f'{prefix}bbox_head.{i}.shared_fcs.0.weight'
        if k in sd:
            sd[k] = sd[k] / 30.0
    return sd


def head_state_dict(roi_head, seed):
    from tests import util
    return _scale_first_layers(util.seeded_state_dict(roi_head, seed=seed), '')


def fixture_state_dict(model, seed):
    return _scale_first_layers(fi.fixture_state_dict(model, seed), 'roi_head.')


def refine_rows(seed, agnostic, C=REFINE_C, rows=REFINE_ROWS):
    """seeded sampled rows of a 2-image batch as one stage hands them to the refinement: rois (N, 5) image-major,
    labels (N) with background (= C) rows, cls_score (N, C+1), bbox_pred (N, 4 | 4C), and per image the pos_is_gt flags
    of its leading positives (ground truths first, as the sampler emits them; image 1 has none)"""
    g = torch.Generator().manual_seed(seed)
    H, W = fi.H, fi.W
    rois, labels, flags = [], [], []
    for b, n in enumerate(rows):
        ctr = torch.rand(n, 2, generator=g) * torch.tensor([W - 3.0, float(H)])
        half = torch.rand(n, 2, generator=g) * torch.tensor([W / 4.0, H / 4.0]) + 2.0
        rois.append(torch.cat([torch.full((n, 1), float(b)), ctr - half, ctr + half], 1))
        n_pos = n // 3
        labels.append(torch.cat([torch.randint(0, C, (n_pos,), generator=g), torch.full((n - n_pos,), C)]))
        f = torch.zeros(n_pos, dtype=torch.uint8)
        if b == 0:
            f[:4] = 1
        flags.append(f)
    N = sum(rows)
    cls_score = torch.randn(N, C + 1, generator=g) * 2
    bbox_pred = torch.randn(N, 4 if agnostic else 4 * C, generator=g) * 1.5
    return torch.cat(rois), torch.cat(labels), cls_score, bbox_pred, flags
