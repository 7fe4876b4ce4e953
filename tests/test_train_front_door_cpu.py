"""not-gpu: the training front door of the multi-scale recipes -- the config rewrite `fuse_device_pipeline(...,
policies=True)` and the host half of `FusedAugResizeNormalizePad` (`plan`: every random draw, box, label and meta)
against the host chain AutoAugment / RandomFlip / Normalize / Pad, exactly."""
import copy
import os

import numpy as np
import pytest

import brcnn  # noqa: F401
from brcnn import Config
from brcnn import pipelines as P
from tests.front_door_util import (ROOT, SHAPES, assert_same_results, chain_cfg, real_policies, sample, same_state,
                                   small_policies)

RECIPES = ['r50_pafpn_mstrain_2x_coco', 'r50_fpn_1x_coco', 'x101_pafpn_mstrain_3x_coco', 'r2_101_fpn_mstrain_3x_coco',
           'r2_101_dcn_pafpn_mstrain_3x_coco', 'r50_pafpn_1x_coco']
FUSED_TYPES = ['LoadImageFromFile', 'LoadAnnotations', 'FusedAugResizeNormalizePad', 'DeviceFormatBundle', 'Collect']


def _train_pipeline(cfg):
    """the pipeline the recipe's train set is built with (below its RepeatDataset wrappers)"""
    tr = cfg.data.train
    while tr['type'] == 'RepeatDataset':
        tr = tr['dataset']
    return tr['pipeline']


@pytest.mark.parametrize('name', RECIPES)
def test_recipe_pipelines_rewrite(name):
    cfg = Config.fromfile(os.path.join(ROOT, f'configs/boosting_rcnn/boosting_rcnn_{name}.py'))
    # r50_fpn_1x_coco states the AutoAugment pipeline as `train_pipeline` but, like the reference's file, leaves the
    # dataset entry with its base's plain pipeline: both are checked
    pipes = [_train_pipeline(cfg), cfg.train_pipeline]
    assert any(c['type'] == 'AutoAugment' for c in cfg.train_pipeline)
    for pipe in pipes:
        before = copy.deepcopy([dict(c) for c in pipe])
        fused = P.fuse_device_pipeline(pipe, policies=True)
        if any(c['type'] == 'AutoAugment' for c in pipe):
            assert [c['type'] for c in fused] == FUSED_TYPES
            f, aug = fused[2], [c for c in pipe if c['type'] == 'AutoAugment'][0]
            # the shipped recipes flip in front of AutoAugment and pad to the image's own size
            assert f['flip_first'] is True and f['flip_ratio'] == 0.5 and f['size_divisor'] == 1
            assert f['policies'] == [[dict(s) for s in pol] for pol in aug['policies']]
            assert f['mean'] == [123.675, 116.28, 103.53] and f['to_rgb'] is True
            t = P.Compose(fused[2:3]).transforms[0]                 # builds from the registry
            assert t.runs_on_device and P.first_device_transform(P.Compose(fused[2:])) == 0
            # without the keyword: today's output (only the format bundle is renamed, AutoAugment stays on the host)
            plain = P.fuse_device_pipeline(pipe)
            assert [c['type'] for c in plain] == [c['type'].replace('DefaultFormatBundle', 'DeviceFormatBundle')
                                                  for c in pipe]
            assert [c for c in plain if c['type'] != 'DeviceFormatBundle'] == \
                [c for c in before if c['type'] != 'DefaultFormatBundle']
        else:
            assert fused == P.fuse_device_pipeline(pipe)
            assert [c['type'] for c in fused] == ['LoadImageFromFile', 'LoadAnnotations', 'FusedResizeNormalizePad',
                                                  'DeviceFormatBundle', 'Collect']
        assert [dict(c) for c in pipe] == before                    # the input config is not modified


def test_keyword_default_and_both_flip_orders():
    tail = [dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]
    for flip_first in (False, True):
        pipe = chain_cfg(small_policies(), flip_first) + tail
        fused = P.fuse_device_pipeline(pipe, 'cuda:0', policies=True)
        assert [c['type'] for c in fused] == ['FusedAugResizeNormalizePad', 'DeviceFormatBundle', 'Collect']
        assert fused[0]['flip_first'] is flip_first and fused[0]['device'] == 'cuda:0' and fused[0]['size_divisor'] == 32
        assert P.fuse_device_pipeline(pipe, 'cuda:0') == P.fuse_device_pipeline(pipe, 'cuda:0', policies=False)
        assert [c['type'] for c in P.fuse_device_pipeline(pipe)][:4] == [c['type'] for c in pipe][:4]
    # the plain run is rewritten as before, with or without the keyword
    plain = [dict(type='Resize', img_scale=(160, 96)), dict(type='RandomFlip', flip_ratio=0.5),
             dict(type='Normalize', mean=[0, 0, 0], std=[1, 1, 1]), dict(type='Pad', size_divisor=32)] + tail
    assert P.fuse_device_pipeline(plain, policies=True) == P.fuse_device_pipeline(plain)


@pytest.mark.parametrize('bad', ['extra_step', 'ratio_range', 'no_override', 'other_transform', 'crop_only', 'pad_val'])
def test_unsupported_policies_stay_on_the_host_unchanged(bad):
    pol = small_policies()
    pipe = chain_cfg(pol, True) + [dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img'])]
    if bad == 'extra_step':
        pol[1].append(dict(type='RandomFlip', flip_ratio=0.5))
    elif bad == 'ratio_range':
        pol[1][0] = dict(type='Resize', img_scale=(30, 200), ratio_range=(0.8, 1.2), keep_ratio=True)
    elif bad == 'no_override':
        pol[1][2].pop('override')
    elif bad == 'other_transform':
        pol[0][0] = dict(type='Pad', size_divisor=8)
    elif bad == 'crop_only':
        pol[0] = [pol[1][1]]
    else:
        pipe[3]['pad_val'] = 5
    before = copy.deepcopy(pipe)
    assert P.fuse_device_pipeline(pipe, policies=True) == before and pipe == before
    if bad != 'pad_val':
        with pytest.raises(ValueError):
            P.FusedAugResizeNormalizePad(pol, mean=[0, 0, 0], std=[1, 1, 1], size_divisor=32)


def _check_plan(policies, flip_first, shape, seeds, size_divisor=32, direction='horizontal'):
    """host chain against `plan` under the same seed: results, None outcomes and the generator's state afterwards"""
    cfg = chain_cfg(policies, flip_first, size_divisor, direction=direction)
    host = P.Compose(cfg)
    fused = P.Compose(P.fuse_device_pipeline(cfg, policies=True)).transforms[0]
    assert isinstance(fused, P.FusedAugResizeNormalizePad)
    seen = dict(none=0, crop=0, plain=0, flip=0)
    for s in seeds:
        a, b = sample(shape, 1000 + s), sample(shape, 1000 + s)
        img = b['img']
        np.random.seed(s)
        ha = host(a)
        state = np.random.get_state()
        np.random.seed(s)
        plan = fused.plan(b)
        assert same_state(state, np.random.get_state()), (shape, s)
        assert b['img'] is img                                       # the pixels are neither read nor replaced
        assert_same_results(ha, None if plan is None else b, (shape, s, flip_first))
        if plan is None:
            seen['none'] += 1
            continue
        # the geometry is the host chain's: final size, padded size, a window inside the intermediate image
        assert plan.new == ha['img_shape'][:2] and plan.pad + (3,) == ha['img'].shape == ha['pad_shape']
        top, left, ch, cw = plan.window
        assert 0 <= top and 0 <= left and ch > 0 and cw > 0 and top + ch <= plan.mid[0] and left + cw <= plan.mid[1]
        flip = ha['flip_direction'] if ha['flip'] else None
        assert (plan.src_flip, plan.flip) == ((flip, None) if flip_first else (None, flip))
        seen['crop' if plan.window != (0, 0) + plan.mid else 'plain'] += 1
        seen['flip'] += flip is not None
    return seen


@pytest.mark.parametrize('flip_first', [True, False])
@pytest.mark.parametrize('allow_negative_crop', [True, False])
def test_plan_equals_host_chain(flip_first, allow_negative_crop):
    total = dict(none=0, crop=0, plain=0, flip=0)
    for shape in SHAPES:
        seen = _check_plan(small_policies(allow_negative_crop), flip_first, shape, range(200))
        for k in seen:
            total[k] += seen[k]
    assert total['crop'] > 50 and total['plain'] > 50 and total['flip'] > 50
    assert (total['none'] > 0) == (not allow_negative_crop)          # rejected samples: only where the crop may reject


@pytest.mark.parametrize('crop_type,crop_size', [('absolute', (20, 30)), ('absolute_range', (17, 33)),
                                                 ('relative', (0.6, 0.7)), ('relative_range', (0.4, 0.5))])
def test_plan_equals_host_chain_per_crop_type(crop_type, crop_size):
    for flip_first in (True, False):
        seen = _check_plan(small_policies(False, crop_type, crop_size), flip_first, (64, 48), range(60),
                           direction=['horizontal', 'vertical', 'diagonal'])
        assert seen['crop'] > 5


def test_plan_equals_host_chain_with_the_recipe_policies():
    """the shipped policies (short sides 480-800, crops of 384-600) and the shipped order and padding"""
    seen = _check_plan(real_policies(), True, (120, 161), range(6), size_divisor=1)
    assert seen['crop'] > 0 and seen['plain'] > 0
