"""shared by test_train_front_door_{cpu,gpu}.py: the small policy pair, sample construction and exact comparison of
what the host chain and the fused transform leave in a results dict"""
import os

import numpy as np

from brcnn import pipelines as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
SHAPES = [(37, 53), (64, 48), (120, 161)]
SMALL_SCALES = [(40, 70), (56, 90)]
# every key the chain sets besides the image: Collect's metas plus what Resize / Pad leave behind
KEYS = P._META_KEYS + ('scale', 'scale_idx', 'keep_ratio', 'pad_fixed_size', 'pad_size_divisor')


def small_policies(allow_negative_crop=True, crop_type='absolute_range', crop_size=(17, 33)):
    return [[dict(type='Resize', img_scale=SMALL_SCALES, multiscale_mode='value', keep_ratio=True)],
            [dict(type='Resize', img_scale=[(30, 200), (44, 200)], multiscale_mode='value', keep_ratio=True),
             dict(type='RandomCrop', crop_type=crop_type, crop_size=crop_size, allow_negative_crop=allow_negative_crop),
             dict(type='Resize', img_scale=SMALL_SCALES, multiscale_mode='value', override=True, keep_ratio=True)]]


def real_policies():
    """the AutoAugment policies of the shipped multi-scale recipe"""
    from brcnn import Config
    cfg = Config.fromfile(os.path.join(ROOT, 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_mstrain_2x_coco.py'))
    aug = [c for c in cfg.data.train.dataset.pipeline if c['type'] == 'AutoAugment']
    return [[dict(s) for s in pol] for pol in aug[0]['policies']]


def chain_cfg(policies, flip_first, size_divisor=32, flip_ratio=0.5, direction='horizontal'):
    """AutoAugment, RandomFlip (in front of it when `flip_first`: the shipped recipes' order), Normalize, Pad"""
    aug = dict(type='AutoAugment', policies=policies)
    flip = dict(type='RandomFlip', flip_ratio=flip_ratio, direction=direction)
    return ([flip, aug] if flip_first else [aug, flip]) + \
        [dict(type='Normalize', mean=MEAN, std=STD, to_rgb=True), dict(type='Pad', size_divisor=size_divisor)]


def sample(shape, seed):
    """a decoded image of `shape` with 0 to 5 boxes inside it, as LoadImageFromFile + LoadAnnotations leave it"""
    rng = np.random.RandomState(seed)
    h, w = shape
    img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    n = rng.randint(0, 6)
    x = np.sort(rng.uniform(0, w, (n, 2)), axis=1)
    y = np.sort(rng.uniform(0, h, (n, 2)), axis=1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32).reshape(n, 4)
    return dict(img=img, img_shape=img.shape, ori_shape=img.shape, img_fields=['img'], filename='x.npy',
                ori_filename='x.npy', gt_bboxes=boxes, gt_labels=rng.randint(0, 4, n).astype(np.int64),
                bbox_fields=['gt_bboxes'])


def same(a, b):
    """exact equality, arrays with their dtype"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def assert_same_results(host, fused, what):
    assert (host is None) == (fused is None), what
    if host is None:
        return
    for k in ('gt_bboxes', 'gt_labels') + KEYS:
        assert same(host[k], fused[k]), (what, k, host[k], fused[k])
