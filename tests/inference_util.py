"""Shared pieces of the inference-API tests: the pipelines and ragged source shapes the plan / kernel cases use, and the
host chain (per-image Compose + collate) they are compared against."""
import copy

import numpy as np

from brcnn import pipelines as P
from brcnn.apis import replace_ImageToTensor
from brcnn.datasets import collate

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
# landscape, small, portrait, odd, portrait again, and the one-pixel image (img_scale plans only)
SHAPES = [(1080, 1920), (480, 640), (300, 200), (75, 113), (640, 427), (1, 1)]
SHAPES_SF = SHAPES[:5] + [(2, 3)]          # scale_factor=0.5 turns a one-pixel image into width 0: the host chain divides by zero


def pipeline(img_scale=None, scale_factor=None, flip=False, flip_direction='horizontal', keep_ratio=True, pad=None,
             norm=None, fmt='ImageToTensor', load='LoadImageFromFile'):
    msfa = dict(type='MultiScaleFlipAug', flip=flip, flip_direction=flip_direction,
                transforms=[dict(type='Resize', keep_ratio=keep_ratio), dict(type='RandomFlip'),
                            dict(type='Normalize', **(norm or NORM)), dict(type='Pad', **(pad or dict(size_divisor=32))),
                            dict(type=fmt, keys=['img']) if fmt == 'ImageToTensor' else dict(type=fmt),
                            dict(type='Collect', keys=['img'])])
    if img_scale is not None:
        msfa['img_scale'] = img_scale
    else:
        msfa['scale_factor'] = scale_factor
    return [dict(type=load), msfa]


def tta_pipeline(**kw):
    return pipeline(img_scale=[(1333, 800), (1000, 600)], flip=True, flip_direction=['horizontal', 'vertical'], **kw)


def sf_pipeline(**kw):
    return pipeline(scale_factor=[0.5, 1.0], keep_ratio=False, pad=dict(size=(1088, 1920)), **kw)


def tail_pipeline(**kw):
    """pad_w % 4 != 0: the kernel's 4-byte-store path"""
    return pipeline(img_scale=(64, 48), pad=dict(size=(64, 67)), **kw)


def random_images(shapes, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def host_chain(pipe, images):
    """what the reference's inference_detector builds on the host: dict(img=[A tensors], img_metas=[A lists])"""
    pipe = copy.deepcopy(list(pipe))
    if isinstance(images[0], np.ndarray):
        pipe[0]['type'] = 'LoadImageFromWebcam'
    compose = P.Compose(replace_ImageToTensor(pipe))
    datas = [compose(dict(img=i) if isinstance(i, np.ndarray) else dict(img_info=dict(filename=i), img_prefix=None))
             for i in images]
    return collate(datas, samples_per_gpu=len(images))


def assert_metas_equal(got, ref):
    assert len(got) == len(ref)
    for ga, ra in zip(got, ref):
        assert len(ga) == len(ra)
        for g, r in zip(ga, ra):
            assert list(g.keys()) == list(r.keys())
            for k in r:
                if k == 'scale_factor':
                    assert g[k].dtype == r[k].dtype == np.float32 and np.array_equal(g[k], r[k]), (k, g[k], r[k])
                elif k == 'img_norm_cfg':
                    assert set(g[k]) == set(r[k]) and g[k]['to_rgb'] == r[k]['to_rgb']
                    for n in ('mean', 'std'):
                        assert g[k][n].dtype == r[k][n].dtype and np.array_equal(g[k][n], r[k][n])
                else:
                    assert type(g[k]) is type(r[k]) and g[k] == r[k], (k, g[k], r[k])
